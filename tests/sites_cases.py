"""Shared by test_sites_host.py and test_gpu_msa_sites.py: what every pair carries at chosen columns
of its centre's multiple alignment (include/meshclust_amd.h, mc_nw_msa_sites) restated in Python
over msa_cases.msa()'s points, and host/variants.hpp ported.

The definition, in msa_cases' terms (w, col, W of a centre of L bytes).  For a pair and the
ascending columns `sites` of its centre's block:
  alleles[s]   byte sites[s] of the pair's row of msa_cases.block
  quals[s]     a base there ('=', 'X', an inserted base in its slot): its quality as aligned; the
               column of a centre base the pair deletes: min(Qs[i - 1] if i > 0, Qs[i] if i < la) with
               i read bases before the gap; a slot the pair leaves empty: 0
Two ways to both: from the words (from_words) and from the rendered row alone (from_row: the n-th
non-gap byte of a row is read base n, so the row gives the read position of every column);
test_sites_host.py holds them equal."""
import numpy as np

import msa_cases as A
import nw_trace_cases as T
import profile_cases as F

LISTS = ["all", "none", "edges", "long", "default"]


def from_words(w, col, words, read, qs, sites):
    """One pair at the columns `sites` of its centre's block -> (alleles, quals), uint8 each."""
    at = {int(c): s for s, c in enumerate(sites)}
    al = np.full(len(sites), A.GAP, np.uint8)
    ql = np.zeros(len(sites), np.uint8)
    la = len(read)
    i = j = 0
    for wd in words:
        n, op = int(wd) >> 4, int(wd) & 15
        if op in (T.OP_EQ, T.OP_X):
            for t in range(n):
                s = at.get(int(col[j + t]))
                if s is not None:
                    al[s], ql[s] = A.char(read[i + t]), qs[i + t]
            i, j = i + n, j + n
        elif op == T.OP_D:
            around = ([int(qs[i - 1])] if i > 0 else []) + ([int(qs[i])] if i < la else [])
            for t in range(n):
                s = at.get(int(col[j + t]))
                if s is not None:
                    ql[s] = min(around) if around else 0
            j += n
        else:
            assert op == T.OP_I and n <= w[j]
            for t in range(n):
                s = at.get(int(col[j]) - int(w[j]) + t)
                if s is not None:
                    al[s], ql[s] = A.char(read[i + t]), qs[i + t]
            i += n
    assert (i, j) == (la, len(col) - 1)
    return al, ql


def from_row(row, is_slot, qs, sites):
    """The same from the pair's rendered row: is_slot[c] says whether column c is an insertion slot
    (channel 7 of the profile)."""
    row = np.frombuffer(row, np.uint8)
    sites = np.asarray(sites, np.int64)
    before = np.concatenate([[0], np.cumsum(row != A.GAP)])  # read bases left of every column
    la = int(before[-1])
    assert la == len(qs)
    al = row[sites].copy()
    ql = np.zeros(len(sites), np.uint8)
    for s, c in enumerate(sites):
        i = int(before[c])
        if row[c] != A.GAP:
            ql[s] = qs[i]
        elif not is_slot[c]:
            around = ([int(qs[i - 1])] if i > 0 else []) + ([int(qs[i])] if i < la else [])
            ql[s] = min(around) if around else 0
    return al, ql


# ---------------------------------------------------------------- host/variants.hpp in Python
def variant_sites(counts, min_frac, min_count):
    """counts: one target's [W, 8] profile -> its variant sites, ascending (uint32)."""
    out = []
    for c in range(len(counts)):
        n = sorted((int(counts[c][k]) for k in (0, 1, 2, 3, 5)), reverse=True)
        D, second = sum(n), n[1]
        if second >= min_count and float(second) >= min_frac * float(D):
            out.append(c)
    return np.array(out, np.uint32)


def haplotypes(strings, min_count):
    """strings: one bytes object per read -> [(string, count)] of those seen min_count times or more,
    by count descending, then by bytes ascending."""
    seen = {}
    for s in strings:
        seen[bytes(s)] = seen.get(bytes(s), 0) + 1
    return sorted(((s, n) for s, n in seen.items() if n >= min_count), key=lambda x: (-x[1], x[0]))


# ---------------------------------------------------------------- the named site lists
_cache = {}


def site_lists(which, name):
    """The list `which` for the strands `name` -> one ascending uint32 array per target."""
    q = A.msa()
    out = []
    for t, (w, col, W, counts, _) in enumerate(F.profiles(name)):
        j = int(q.targets[t])
        if which == "all":
            s = np.arange(W)
        elif which == "none":
            s = []
        elif which == "edges":
            s = {0, W - 1} if W else set()
            if j == q.slots:
                s |= set(np.nonzero(counts[:, 7])[0].tolist())
            s = sorted(s)
        elif which == "long":
            s = []
            if j == q.long_target:
                r = int(np.argmax(w))  # (the run of 70 on the plus strand; whatever is longest on the other)
                s0 = int(col[r]) - int(w[r])
                s = ([int(col[r - 1])] if r else []) + [s0 + d for d in (0, 1, 62, 63, 64, 65, 69) if d < w[r]] + ([int(col[r])] if r < len(w) - 1 else [])
        else:
            assert which == "default"
            s = variant_sites(counts, 0.05, 1)
        out.append(np.array(s, np.uint32))
    return out


def flat(lists):
    """-> (site_off[nt + 1] uint64, sites uint32): mc_nw_msa_sites' arguments."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.uint64)
    return off, (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.uint32)


def pair_inputs(name):
    """Per pair of msa_cases.msa() for the strands `name`: (target index, words, read and qualities
    as aligned); computed once per process."""
    if ("i", name) not in _cache:
        q = A.msa()
        am = q.strands(name)
        exp = A.expected()
        ql = F.qualities()
        out = []
        for k in range(len(q.a)):
            x = ql[q.a[k]]
            out.append((q.tindex[int(q.b[k])], exp[am[k]][k][0], q.read(k, bool(am[k])), x[::-1] if am[k] else x))
        _cache[("i", name)] = out
    return _cache[("i", name)]


def expected(which, name):
    """-> (site_off, sites, off[m + 1], alleles, quals) of all pairs, mc_nw_msa_sites' layout, from the
    words; computed once per process and left unchanged."""
    if ("e", which, name) not in _cache:
        lists = site_lists(which, name)
        pr = F.profiles(name)
        al, ql = [], []
        for t, words, read, qs in pair_inputs(name):
            x, y = from_words(pr[t][0], pr[t][1], words, read, qs, lists[t])
            al.append(x)
            ql.append(y)
        off = np.concatenate([[0], np.cumsum([len(x) for x in al])]).astype(np.uint64)
        so, st = flat(lists)
        res = (so, st, off, np.concatenate(al).astype(np.uint8), np.concatenate(ql).astype(np.uint8))
        for x in res:
            x.setflags(write=False)
        _cache[("e", which, name)] = res
    return _cache[("e", which, name)]
