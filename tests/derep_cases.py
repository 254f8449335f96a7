"""The points and the expectations of the dereplication tests (mc_derep, host/derep.hpp).

One seeded set of points, built as raw byte strings for ``load_sequences``, and a Python restatement of
the definition: a dict keyed by ``min(s, rc(s))`` under rc_byte's rule (host/revseq.hpp) gives ``rep``
and ``minus`` for any id list.  Nothing here touches the code under test.

Per length of LENGTHS a base string (digits 0..3) and: an exact copy, a minus-strand copy, copies that
differ in the first, a middle and the last byte only, the string without its last byte, the string plus one
byte.  Then strings that are their own minus strand with a copy, a read with 'N' inside (copy, minus-strand
copy, the run of N replaced by bases), a raw-letter record (its letter reverse complement; the same bases as
digits, which is no duplicate), a class of four in the order rc(a), a, a, rc(a), and one string copied to
every start offset mod 16 behind fillers."""
import functools

import numpy as np

LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 70001)
N = ord("N")

_RC = np.arange(256, dtype=np.uint8)
_RC[:4] = [3, 2, 1, 0]
for _a, _b in ("AT", "CG"):
    _RC[ord(_a)], _RC[ord(_b)] = ord(_b), ord(_a)


def rc(s):
    """the minus-strand string: reversed, digits d -> 3 - d, A <-> T, C <-> G, anything else unchanged"""
    return _RC[np.asarray(s, np.uint8)[::-1]].copy()


class Cases:
    def __init__(self):
        rng = np.random.default_rng(317)
        self.points, self.kind, self.group = [], [], []  # group: (what, length) of the base string it derives from

        def add(s, kind, group):
            self.points.append(np.ascontiguousarray(s, np.uint8))
            self.kind.append(kind)
            self.group.append(group)
            return len(self.points) - 1

        def other(v):
            return np.uint8((int(v) + 1 + int(rng.integers(0, 3))) % 4)

        for L in LENGTHS:
            g = ("len", L)
            base = rng.integers(0, 4, L).astype(np.uint8)
            add(rng.integers(0, 4, int(rng.integers(1, 20))), "filler", g)  # (moves the group's start offset)
            add(base, "base", g)
            add(base.copy(), "copy", g)
            add(rc(base), "minus", g)
            if L >= 1:
                for kind, at in (("first", 0), ("middle", L // 2), ("last", L - 1)):
                    s = base.copy()
                    s[at] = other(s[at])
                    add(s, kind, g)
                add(base[:-1], "shorter", g)
            add(np.append(base, np.uint8(rng.integers(0, 4))), "longer", g)
        for half in (1, 32, 500):  # their own minus strand: lengths 2, 64, 1000
            h = rng.integers(0, 4, half).astype(np.uint8)
            s = np.concatenate([h, rc(h)])
            g = ("self", 2 * half)
            add(s, "base", g)
            add(rng.integers(0, 4, 3), "filler", g)
            add(s.copy(), "copy", g)
        g = ("N", 90)
        s = rng.integers(0, 4, 90).astype(np.uint8)
        s[30:42] = N  # (a run the FASTA parser keeps as 'N' on either strand: 10 or more, 20 bases or more on both sides)
        add(s, "base", g)
        add(s.copy(), "copy", g)
        add(rc(s), "minus", g)
        t = s.copy()
        t[30:42] = rng.integers(0, 4, 12)
        add(t, "n_replaced", g)
        g = ("letters", 50)
        d = rng.integers(0, 4, 50).astype(np.uint8)
        letters = np.frombuffer(b"ACGT", np.uint8)[d]
        add(letters, "base", g)
        add(rc(letters), "minus", g)
        add(letters.copy(), "copy", g)
        add(d, "digits", g)  # the same bases as digits: other bytes, no duplicate
        g = ("four", 100)
        a = rng.integers(0, 4, 100).astype(np.uint8)
        for s, kind in ((rc(a), "base"), (a, "minus"), (a.copy(), "minus"), (rc(a), "copy")):
            add(s, kind, g)
        g = ("offsets", 40)
        a = rng.integers(0, 4, 40).astype(np.uint8)
        add(a, "base", g)
        for r in range(32):  # a copy at every start offset mod 16, as written and minus
            cur = sum(len(p) for p in self.points) % 16
            add(rng.integers(0, 4, (r - cur) % 16 or 16), "filler", g)
            add(rc(a) if r >= 16 else a.copy(), "minus" if r >= 16 else "copy", g)
        self.n = len(self.points)
        self.lens = np.array([len(p) for p in self.points], np.uint64)
        self.seq_off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.codes = np.concatenate(self.points).astype(np.uint8)
        self._bytes = [p.tobytes() for p in self.points]
        self._rcbytes = [rc(p).tobytes() for p in self.points]

    def load_args(self):
        """codes, seq_off, seg, seg_off for Engine.load_sequences: a segment per maximal run of digits"""
        seg, seg_off = [], [0]
        for p in self.points:
            dig = np.concatenate([[0], (p <= 3).astype(np.int8), [0]])
            edges = np.nonzero(np.diff(dig))[0]
            for s, e in zip(edges[::2], edges[1::2]):
                seg += [int(s), int(e) - 1]
            seg_off.append(len(seg) // 2)
        return self.codes, self.seq_off, np.array(seg, np.int32), np.array(seg_off, np.uint64)

    def expected(self, ids, strands):
        """the restatement: (rep, minus) of mc_derep for the id list and strands 1 or 3"""
        first = {}
        rep = np.zeros(len(ids), np.uint32)
        minus = np.zeros(len(ids), np.uint8)
        for i, p in enumerate(ids):
            s = self._bytes[int(p)]
            key = min(s, self._rcbytes[int(p)]) if strands == 3 else s
            j = first.setdefault(key, i)
            rep[i] = j
            minus[i] = 0 if s == self._bytes[int(ids[j])] else 1
        return rep, minus


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()


def classes(rep):
    """derep_classes: (first position, size) of every class, size descending, then first position ascending"""
    rep = np.asarray(rep, np.int64)
    size = np.bincount(rep, minlength=len(rep))
    firsts = [int(i) for i in np.nonzero(rep == np.arange(len(rep)))[0]]
    return sorted(((i, int(size[i])) for i in firsts), key=lambda t: (-t[1], t[0]))


# ---------------------------------------------------------------- the tool's input and its expected files
_LET = np.frombuffer(b"ACGT", np.uint8)
_CMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def letters(p):
    return "".join(chr(_LET[v]) if v <= 3 else chr(v) for v in p)


def tool_reads():
    """(name, sequence as written in the file) for the tool: the cases of A, C, G, T and N of 2 .. 300 bases (the parser refuses a record of one base),
    some written in lower case"""
    c = cases()
    out = []
    for i, p in enumerate(c.points):
        if 2 <= len(p) <= 300 and c.group[i][0] != "letters" and c.kind[i] != "filler":
            s = letters(p)
            out.append(("r%d_%s" % (i, c.kind[i]), s.lower() if len(out) % 3 == 1 else s))
    return out


def tool_expected(reads, both, min_size=1):
    """the bytes of --output and --table for reads [(name, sequence)]"""
    up = [s.upper() for _, s in reads]
    rcl = lambda s: "".join(_CMP[ch] for ch in reversed(s))
    first, rep, minus = {}, [], []
    for i, s in enumerate(up):
        j = first.setdefault(min(s, rcl(s)) if both else s, i)
        rep.append(j)
        minus.append(0 if s == up[j] else 1)
    size = np.bincount(rep, minlength=len(rep))
    fa = "".join(">%s;size=%d\n%s\n" % (reads[i][0], n, up[i]) for i, n in classes(rep) if n >= min_size)
    tab = "".join("%s\t%s\t%s\t%d\n" % (reads[i][0], reads[rep[i]][0], "-" if minus[i] else "+", size[rep[i]]) for i in range(len(reads)))
    stats = dict(reads=len(reads), uniques=len(set(rep)), written=sum(1 for _, n in classes(rep) if n >= min_size),
                 largest=int(size.max()), minus=int(sum(minus)), strands=3 if both else 1)
    return fa.encode(), tab.encode(), stats


def fasta_text(reads):
    return "".join(">%s\n%s\n" % r for r in reads)


def fastq_text(reads):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in reads)
