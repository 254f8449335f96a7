"""Deterministic scripts over the get_close / mean-shift step API (mc_set_order, mc_kill,
mc_cluster_begin, mc_scan, mc_scan_part, mc_scan_commit, mc_align_part, mc_scan_ident, mc_mean_shift,
mc_mean_shift_range), run call by call on any engine with the C-ABI of include/meshclust_amd.h.

The GPU tests (test_gpu_steps.py) run a script on libmcgpu and on the CPU oracle engine
(oracle/_build/libmcoracle_engine.so, the serial double-precision restatement of every call) and
compare the two traces exactly; test_step_scenarios_host.py runs the scripts on the oracle engine
alone and checks that the inputs reach the cases they were built for (ties of the first maximum
across lanes, waves and workgroups; get_mean ties whose push order disagrees with the position
order; flagged shares that split; the sizes at which the kernels change path).

A trace is a list of (tag, dict) records holding every return code, every mc_scan_result field,
every flagged list, identity array, pairs / cells count and new-centre array.  Doubles are kept
as bit patterns (NaN as "nan"), so equality of traces is bit-for-bit equality.  Two fields are
kept only where the header defines them: best_pos / best_val where has_best is set (no maximum
exists otherwise), new_centre where the step was not is_min.
"""
import os

import numpy as np

import fixtures
import meshclust_amd as M
import oracle_lib as O

ROOT = os.path.dirname(fixtures.HERE)
ORACLE_ENGINE = os.path.join(ROOT, "oracle", "_build", "libmcoracle_engine.so")
BLOCK = 256  # MC_SHARD_BLOCK, and the scan kernels' workgroup
OFFSETS = (0, 1, 64, 256, 513)  # copies of one read: the next lane, the next wave, the next workgroups

# name -> k, histogram width, reads, classifier, and what the row is there for
ROWS = {
    "k3w1": dict(k=3, width=1, n=1500, cls="a1k"),             # nch = 4; a step flagging >= 300 (unrolled add_rows)
    "k4w1": dict(k=4, width=1, n=1000, cls="two"),            # nch == 16
    "k5w1": dict(k=5, width=1, n=1000, cls="one"),            # nch = 64: row-per-wave mean_closest_fast, short add_rows
    "k6w1": dict(k=6, width=1, n=1500, cls="one"),            # nch = 256: general add_rows
    "k7w1": dict(k=7, width=1, n=257, cls="one"),             # B = 16384: column sums in global memory
    "k3w2": dict(k=3, width=2, n=1000, cls="two"),            # 16-bit bins
    "k6w2": dict(k=6, width=2, n=257, cls="one"),             # 16-bit bins, B = 4096
    "k2w4": dict(k=2, width=4, n=4400, cls="one", wide=True, big=4120, unrelated=20),  # non-fused path, > 4096 flagged
}
FUSED = [r for r in ROWS if not ROWS[r].get("wide")]

_cpu = None


def oracle_engine():
    """A new context of the CPU oracle engine (ctypes' default RTLD_LOCAL, beside libmcgpu)."""
    global _cpu
    if _cpu is None:
        _cpu = M.load_engine_lib(ORACLE_ENGINE)
    return M.Engine(0, lib=_cpu)


# ------------------------------------------------------------------------------------ inputs
class Input:
    pass


def _mutate(rng, s, nsub):
    t = s.copy()
    q = rng.choice(len(s), size=nsub, replace=False)
    t[q] = (t[q] + rng.integers(1, 4, size=nsub)) % 4
    return t.astype(np.uint8)


def make_input(row, seed=None):
    """Reads of 120-300 bases (100 in the wide row), one segment each: families of a template with
    3-40 exact copies and mutants of 1-15 % substitutions, plus unrelated reads; and the static
    order, with the copies of six families at p, p + 1, p + 64, p + 256, p + 513 and the family's
    first point (the one the walk starts its cluster from) above them, at the top of the order."""
    spec = ROWS[row]
    n = spec["n"]
    rng = np.random.default_rng(1000 + sorted(ROWS).index(row) if seed is None else seed)
    lo, hi = (100, 100) if spec.get("wide") else (120, 300)
    reads, fam, kind = [], [], []  # kind: 0 copy, 1 mutant, 2 unrelated
    families = []
    big = spec.get("big", n // 4)  # family 0: large, of very light mutants (one step flags them all)
    budget = n - spec.get("unrelated", n // 12)
    mut_hi = 13 if spec.get("wide") else 30
    f = 0
    while True:
        L = int(rng.integers(lo, hi + 1))
        tmpl = rng.integers(0, 4, size=L).astype(np.uint8)
        ncopy = int(rng.integers(6, 13)) if f < 6 else int(rng.integers(3, 41))
        nmut = 0 if f in (2, 5) else int(rng.integers(6, mut_hi))  # families 2 and 5: copies only
        light = 0
        if f == 0:
            ncopy, nmut, light = 40, 12, big - 52
        if f >= 6 and len(reads) + ncopy + nmut > budget:
            break
        ids = {"copies": [], "mutants": [], "graded": nmut}
        for _ in range(ncopy):
            ids["copies"].append(len(reads))
            reads.append(tmpl.copy())
            fam.append(f)
            kind.append(0)
        for j in range(nmut + light):
            rate = (0.01, 0.03, 0.06, 0.10, 0.15)[j % 5]
            nsub = max(1, int(round(rate * L))) if j < nmut else int(rng.integers(1, 3))
            ids["mutants"].append(len(reads))
            reads.append(_mutate(rng, tmpl, nsub))
            fam.append(f)
            kind.append(1)
        families.append(ids)
        f += 1
    assert len(reads) < n
    while len(reads) < n:
        reads.append(rng.integers(0, 4, size=int(rng.integers(lo, hi + 1))).astype(np.uint8))
        fam.append(-1)
        kind.append(2)
    # shuffle the ids, so that id order says nothing about families
    perm = rng.permutation(n)
    inv = np.argsort(perm)
    reads = [reads[i] for i in perm]
    fam = np.array(fam)[perm]
    kind = np.array(kind)[perm]
    for ids in families:
        ids["copies"] = [int(inv[i]) for i in ids["copies"]]
        ids["mutants"] = [int(inv[i]) for i in ids["mutants"]]
    # the static order
    slots = {}
    bases = (5, 17, 100, 150, 230, 40) if n >= 1000 else (0, 20, 40, 60, 130, 150)
    for j in range(6):
        cp = families[j]["copies"]
        # families 1 and 4 start from a light mutant: the tied copies then come from the steps
        # alone; the others start from a copy: the first member ties with its copies
        first = families[j]["mutants"][0] if j in (1, 4) else cp[-1]
        slots[n - 1 - j] = first
        t = 0
        for o in OFFSETS:
            if bases[j] + o < n - 8 and t < len(cp) - 1:
                slots[bases[j] + o] = cp[t]
                t += 1
    used = set(slots.values())
    rest = [i for i in rng.permutation(n) if int(i) not in used]
    order = np.zeros(n, np.uint32)
    it = iter(rest)
    for p in range(n):
        order[p] = slots[p] if p in slots else next(it)
    assert sorted(order.tolist()) == list(range(n))
    inp = Input()
    inp.row, inp.k, inp.width, inp.n, inp.spec = row, spec["k"], spec["width"], n, spec
    inp.reads, inp.fam, inp.kind, inp.families, inp.order = reads, fam, kind, families, order
    inp.pos = np.argsort(order).astype(np.int64)  # pos[id]
    inp.codes = np.concatenate(reads)
    inp.seq_off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    inp.seg = np.array([[0, len(r) - 1] for r in reads], np.int32).reshape(-1)
    inp.seg_off = np.arange(n + 1, dtype=np.uint64)
    return inp


def load(eng, inp):
    eng.load_sequences(inp.codes, inp.seq_off, inp.seg, inp.seg_off)
    eng.kmer_build(inp.k, inp.width)


def _template_pairs(inp):
    a, b = [], []
    for ids in inp.families:
        for m in ids["mutants"][:ids["graded"]]:  # (not family 0's very light ones)
            a.append(m)
            b.append(ids["copies"][0])
    return np.array(a, np.uint32), np.array(b, np.uint32)


def make_classifier(inp, ref):
    """The row's classifier.  "a1k": the trained one of tests/golden/train_a1k.npz.  "one": the
    intersection feature alone against a threshold; "two": intersection and Manhattan distance, two
    combos.  The thresholds are medians of the oracle engine's (``ref``, loaded) own values over
    the (mutant, template) pairs, so that about half of the mutants are similar."""
    kindc = inp.spec["cls"]
    if kindc == "a1k":
        return O.classifier_from_golden(np.load(fixtures.golden("train_a1k.npz")))
    a, b = _template_pairs(inp)
    c = O.Classifier()
    if kindc == "one":
        raw = ref.pair_features(a, b, [M.FEAT_INTERSECTION])
        c.n_single = 1
        c.lookup[0], c.is_sim[0], c.mins[0], c.maxs[0] = M.FEAT_INTERSECTION, 1, 0.0, 1.0
        c.n_combo = 1
        c.combo_kind[0], c.combo_len[0] = M.COMBO_SELF, 1
        c.combo_idx[0][0] = 0
        c.weights[0], c.weights[1] = -float(np.median(raw[:, 0])), 1.0
        return c
    raw = ref.pair_features(a, b, [M.FEAT_INTERSECTION, M.FEAT_MANHATTAN])
    far = ref.pair_features(a, np.roll(b, 7), [M.FEAT_MANHATTAN])
    mx = float(max(raw[:, 1].max(), far[:, 0].max()))
    c.n_single = 2
    c.lookup[0], c.is_sim[0], c.mins[0], c.maxs[0] = M.FEAT_INTERSECTION, 1, 0.0, 1.0
    c.lookup[1], c.is_sim[1], c.mins[1], c.maxs[1] = M.FEAT_MANHATTAN, 0, 0.0, mx
    c.n_combo = 2
    c.combo_kind[0], c.combo_len[0] = M.COMBO_SELF, 1
    c.combo_idx[0][0] = 0
    c.combo_kind[1], c.combo_len[1] = M.COMBO_SQUARED, 2
    c.combo_idx[1][0], c.combo_idx[1][1] = 0, 1
    c0 = raw[:, 0]
    c1 = (c0 * c0) * ((1 - raw[:, 1] / mx) ** 2)
    c.weights[0], c.weights[1], c.weights[2] = -float(np.median(c0 + c1)), 1.0, 1.0
    return c


def align_classifier(cutoff):
    """The classifier Trainer::train installs in alignment mode (Trainer.cpp:570-577)."""
    c = O.Classifier()
    c.n_single = 1
    c.lookup[0], c.is_sim[0], c.mins[0], c.maxs[0] = M.FEAT_ALIGN, 1, 0.0, 1.0
    c.n_combo = 1
    c.combo_kind[0], c.combo_len[0] = M.COMBO_SELF, 1
    c.combo_idx[0][0] = 0
    c.weights[0], c.weights[1] = -cutoff, 1.0
    return c


# ------------------------------------------------------------------------------------ traces
def _bits(x):
    x = np.float64(x)
    return "nan" if np.isnan(x) else int(x.view(np.uint64))


def _bits_arr(a):
    return tuple(_bits(x) for x in np.asarray(a, np.float64))


def _res(rc, r, part=False):
    d = {"rc": rc}
    if rc != 0:
        return d
    for key in ("is_min", "has_best", "n_flagged", "n_members", "nw_pairs", "nw_cells"):
        d[key] = int(r[key])
    d["best_pos"] = int(r["best_pos"]) if r["has_best"] else None
    d["best_val"] = _bits(r["best_val"]) if r["has_best"] else None
    d["new_centre"] = int(r["new_centre"]) if not r["is_min"] or part else None
    return d


class Run:
    """One engine running a script: the trace, and the driver's own mirror of the bvec and of the
    cluster (built from what the engine returned), which the host-side condition checks read."""

    def __init__(self, eng, inp):
        self.eng, self.inp = eng, inp
        self.trace, self.steps = [], []
        self.reset()

    def rec(self, tag, **kw):
        self.trace.append((tag, kw))

    def reset(self):
        self.rec("set_order", rc=self.eng.set_order(self.inp.order))
        self.alive = np.ones(self.inp.n, bool)
        self.members = []

    def kill(self, pos):
        self.rec("kill", pos=int(pos), rc=self.eng.kill(pos))
        self.alive[pos] = False

    def begin(self, first):
        self.rec("cluster_begin", first=int(first), rc=self.eng.cluster_begin(first))
        self.members = [int(first)]

    def _applied(self, kind, centre, S, E, cand, d, fl):
        self.alive[fl] = False
        self.members += [int(self.inp.order[p]) for p in fl]
        self.steps.append(dict(kind=kind, centre=int(centre), S=int(S), E=int(E), cand=cand, res=d,
                               flagged=np.array(fl, np.int64), members=list(self.members)))

    def scan(self, centre, S, E):
        cand = np.nonzero(self.alive[S:E + 1])[0] + S
        rc, r, fl = self.eng.scan(centre, S, E)
        d = _res(rc, r)
        self.rec("scan", centre=int(centre), S=int(S), E=int(E), flagged=tuple(int(x) for x in fl), **d)
        if rc == 0:
            self._applied("scan", centre, S, E, cand, d, fl)
        return d

    def parts(self, centre, S, E, nparts):
        """mc_scan_part for every part -> the parts combined by the header's rule (is_min AND, the
        largest best_val, ties to the lowest best_pos, flagged lists merged)."""
        best, merged, is_min = None, [], 1
        for part in range(nparts):
            rc, r, fl = self.eng.scan_part(centre, S, E, part, nparts)
            d = _res(rc, r, part=True)
            self.rec("scan_part", centre=int(centre), S=int(S), E=int(E), part=part, nparts=nparts,
                     flagged=tuple(int(x) for x in fl), **d)
            if rc != 0:
                return None
            is_min &= d["is_min"]
            merged += [int(x) for x in fl]
            if d["has_best"]:
                v, p = float(r["best_val"]), d["best_pos"]
                if best is None or v > best[0] or (v == best[0] and p < best[1]):
                    best = (v, p, d["best_val"])
        merged.sort()
        return dict(is_min=is_min, has_best=int(best is not None), best_pos=best[1] if best else None,
                    best_val=best[2] if best else None, flagged=tuple(merged))

    def commit(self, centre, S, E, merged):
        cand = np.nonzero(self.alive[S:E + 1])[0] + S
        rc, r = self.eng.scan_commit(np.array(merged, np.uint32))
        d = _res(rc, r)
        self.rec("scan_commit", flagged=tuple(merged), **d)
        if rc == 0:
            self._applied("commit", centre, S, E, cand, d, np.array(merged, np.int64))
        return d


def windows(inp, run):
    """The walk's windows, taken in turn: the whole order, single block boundaries, single
    positions, mid-block to mid-block across three blocks, and one whose candidates are all dead."""
    n = inp.n
    dead = np.nonzero(~run.alive)[0]
    dw = None
    if len(dead):  # the longest run of dead positions
        brk = np.nonzero(np.diff(dead) != 1)[0]
        starts = np.concatenate([[0], brk + 1])
        ends = np.concatenate([brk, [len(dead) - 1]])
        i = int(np.argmax(ends - starts))
        dw = (int(dead[starts[i]]), int(dead[ends[i]]))
    mid = (100, min(700, n - 2))
    return [(0, n - 1), (256, min(511, n - 1)), mid, (0, n - 1), (255, 256), (n // 2, n - 1), (n // 4, n - 1), (0, n - 1),
            (1, 1), (0, n // 2), (0, max(n - 200, n // 2 + 30)), (0, n - 1), (n - 1, n - 1), dw, (64, 64 + n // 3), (0, n - 1)]


# where cluster c starts in the window list: the whole order, or a run of growing windows (so that
# a cluster grows over several steps, the earlier ones at higher positions), or one of the small ones
STARTS = (0, 1, 5, 9, 14, 5, 9, 14, 4, 5, 8, 9, 12, 14, 13, 1)


def run_walk(eng, inp, max_clusters=40, sharded=True):
    """(a) The accumulation-like walk: cluster_begin(first) with first the point at the highest
    alive position, kill of that position, then scans with centre = new_centre until is_min.
    Cluster c takes its windows in turn starting from entry STARTS[c % 16].  Before
    three of the steps nine kills in a row are made, inside and outside the next window (the
    deferred kills: eight pending, flushed on the ninth); once a kill is followed by a sharded
    step (mc_scan_part x 2 + mc_scan_commit in the place of mc_scan)."""
    run = Run(eng, inp)
    nstep, did_shard = 0, not sharded
    for c in range(max_clusters):
        al = np.nonzero(run.alive)[0]
        if not len(al):
            break
        fpos = int(al[-1])
        first = int(inp.order[fpos])
        run.begin(first)
        run.kill(fpos)
        centre, w = first, STARTS[c % len(STARTS)]
        while True:
            win = windows(inp, run)
            S, E = win[w % len(win)] or win[(w + 1) % len(win)]
            w += 1
            nstep += 1
            if nstep in (2, 9, 23):
                al = np.nonzero(run.alive)[0]
                inside = [int(p) for p in al if S <= p <= E][1::3][:5]
                outside = [int(p) for p in al if p < S or p > E][::5]
                outside += [int(p) for p in al if p not in inside][::7]
                for p in (inside + [p for p in outside if p not in inside])[:9]:
                    run.kill(p)
            if nstep >= 5 and not did_shard and run.alive[S:E + 1].sum() > 2:
                did_shard = True
                run.kill(int(np.nonzero(run.alive[S:E + 1])[0][1]) + S)
                comb = run.parts(centre, S, E, 2)
                if comb is None:
                    return run
                d = run.commit(centre, S, E, comb["flagged"])
            else:
                d = run.scan(centre, S, E)
            if d["rc"] != 0:
                return run
            if d["is_min"]:
                break
            centre = d["new_centre"]
    return run


def _prelude(run, inp, fam, second):
    """A new cluster from family ``fam``'s first point; with ``second`` its first step too."""
    n = inp.n
    fpos = n - 1 - fam
    run.begin(int(inp.order[fpos]))
    run.kill(fpos)
    for p in (3, 300 % n, n // 2):  # pending kills travel into the step
        run.kill(p)
    centre = int(inp.order[fpos])
    if second:
        d = run.scan(centre, n // 2, n - 1)
        if d["rc"] == 0 and not d["is_min"]:
            centre = d["new_centre"]
    return centre


def run_sharded(eng, inp):
    """(b) The same step as mc_scan and as mc_scan_part for every part of nparts in {1, 2, 3, 5, 7}
    + mc_scan_commit of the merged list, each from a replayed state (mc_set_order + the same
    prelude): a new cluster's step and a grown cluster's, over the whole order and over a window
    from mid-block to mid-block (three blocks: with 5 and 7 parts some parts own no block).
    Returns (run, cases): cases[i] = (the mc_scan record, [(combined parts, commit record)])."""
    run = Run(eng, inp)
    n = inp.n
    cases = []
    for fam, second, (S, E) in ((0, False, (0, n - 1)), (1, True, (0, n - 1)), (3, False, (100, min(700, n - 2))),
                                (0, True, (100, min(700, n - 2)))):
        run.reset()
        centre = _prelude(run, inp, fam, second)
        whole = run.scan(centre, S, E)
        whole = dict(whole, flagged=tuple(int(x) for x in run.steps[-1]["flagged"]))
        variants = []
        for nparts in (1, 2, 3, 5, 7):
            run.reset()
            centre = _prelude(run, inp, fam, second)
            comb = run.parts(centre, S, E, nparts)
            if comb is None:
                return run, cases
            variants.append((comb, run.commit(centre, S, E, comb["flagged"])))
        cases.append((whole, variants))
    # a commit of nothing on a fresh cluster, then a step of the same cluster
    run.reset()
    run.begin(int(inp.order[n - 1]))
    run.kill(n - 1)
    run.commit(int(inp.order[n - 1]), 0, n - 1, [])
    run.scan(int(inp.order[n - 1]), 0, n - 1)
    return run, cases


def check_sharded(cases):
    """The parts, combined by the header's rule, are the whole step; the commit gives its cluster."""
    assert len(cases) == 4
    for whole, variants in cases:
        assert whole["rc"] == 0 and whole["n_flagged"] > 0
        assert len(variants) == 5
        for comb, commit in variants:
            for key in ("is_min", "has_best", "best_pos", "best_val", "flagged"):
                assert comb[key] == whole[key], key
            assert commit["rc"] == 0
            assert (commit["new_centre"], commit["n_members"]) == (whole["new_centre"], whole["n_members"])


def run_msum(eng, inp, through_parts):
    """(e) A cluster whose first step flags nothing and whose second step, with no
    mc_cluster_begin in between, does: after another cluster has left its column sums behind."""
    run = Run(eng, inp)
    n = inp.n

    def step(centre, S, E):
        if not through_parts:
            return run.scan(centre, S, E)
        comb = run.parts(centre, S, E, 2)
        return run.commit(centre, S, E, comb["flagged"])

    for fam in (3, 0):  # a cluster grown the usual way first
        fpos = n - 1 - fam
        first = int(inp.order[fpos])
        run.begin(first)
        run.kill(fpos)
        if fam == 0:
            quiet = int(np.nonzero(run.alive & (inp.kind[inp.order] == 2))[0][0])  # an unrelated read
            d = step(first, quiet, quiet)
            assert d["rc"] != 0 or d["is_min"], "the quiet window flagged something"
        centre = first
        for _ in range(3):
            d = step(centre, 0, n - 1)
            if d["rc"] != 0 or d["is_min"]:
                break
            centre = d["new_centre"]
    return run


def run_align(eng, inp, cutoff, max_clusters=5):
    """(c) Alignment mode: a short walk with mc_scan, every other step instead as mc_align_part
    for nparts in {1, 2, 3} (pairs and cells on every part), the parts of nparts = 3 interleaved
    back and given to mc_scan_ident."""
    run = Run(eng, inp)
    n = inp.n
    nstep = 0
    for c in range(max_clusters):
        al = np.nonzero(run.alive)[0]
        fpos = int(al[-1])
        first = int(inp.order[fpos])
        run.begin(first)
        run.kill(fpos)
        centre = first
        for S, E in ((n // 2, n - 1), (0, n - 1), (3, n - 2), (0, n - 1)):
            nstep += 1
            if (nstep + c) % 2 == 0:
                cand = np.nonzero(run.alive[S:E + 1])[0] + S
                ident = np.zeros(len(cand))
                for nparts in (1, 2, 3):
                    for part in range(nparts):
                        rc, idn, pairs, cells = eng.align_part(centre, S, E, part, nparts)
                        run.rec("align_part", centre=centre, S=S, E=E, part=part, nparts=nparts, rc=rc, ident=_bits_arr(idn),
                                pairs=pairs, cells=cells)
                        if rc != 0:
                            return run
                        if nparts == 3:
                            ident[part::3] = idn
                rc, r, fl = eng.scan_ident(centre, S, E, ident)
                d = _res(rc, r)
                run.rec("scan_ident", centre=centre, S=S, E=E, flagged=tuple(int(x) for x in fl), **d)
                if rc == 0:
                    run._applied("scan_ident", centre, S, E, cand, d, fl)
            else:
                d = run.scan(centre, S, E)
            if d["rc"] != 0:
                return run
            if d["is_min"]:
                break
            centre = d["new_centre"]
    return run


def mean_shift_cases(inp):
    """(d) CSR member lists: whole families in input order (exact copies side by side), clusters of
    one point, a family split over two neighbouring clusters; centres that are members, and one
    that is not."""
    fams = [ids["copies"] + ids["mutants"][:10] for ids in inp.families[1:9]]
    lists = []
    for i, f in enumerate(fams):
        if i % 3 == 0:
            lists += [f[:len(f) // 2], f[len(f) // 2:]]
        else:
            lists.append(f)
        if i % 2 == 1:
            lists.append([int(np.nonzero(inp.kind == 2)[0][i])])
    members = np.array([x for l in lists for x in l], np.uint32)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    centres = np.array([l[-1] for l in lists], np.uint32)
    centres[2] = int(np.nonzero(inp.kind == 2)[0][0])
    return centres, off, members


def run_mean_shift(eng, inp):
    centres, off, members = mean_shift_cases(inp)
    C_ = len(centres)
    trace = []
    for delta in (0, 2, C_):
        try:
            out = eng.mean_shift(centres, off, members, delta)
            trace.append(("mean_shift", dict(delta=delta, rc=0, new=tuple(int(x) for x in out))))
        except M.MCError as e:
            trace.append(("mean_shift", dict(delta=delta, rc=e.code)))
        for j0, j1 in ((0, C_), (0, 0), (C_, C_), (0, 5), (5, C_), (3, C_ - 2)):
            rc, out = eng.mean_shift_range(centres, off, members, delta, j0, j1)
            trace.append(("mean_shift_range", dict(delta=delta, j0=j0, j1=j1, rc=rc,
                                                   new=tuple(int(x) for x in out) if rc == 0 else None)))
    return trace


def run_errors(eng, inp):
    """(f) Return codes alone: a flagged buffer one short (mc_set_order again after it: the
    context's bvec state is undefined then), S > E, E >= n, part >= nparts, a commit of a dead
    position and of descending positions."""
    run = Run(eng, inp)
    n = inp.n
    first = int(inp.order[n - 1])
    run.begin(first)
    run.kill(n - 1)
    d = run.scan(first, 0, n - 1)
    nf = d["n_flagged"]
    assert nf >= 2
    run.reset()
    run.begin(first)
    run.kill(n - 1)
    fused = not inp.spec.get("wide")
    rcs = [("cap", eng.scan(first, 0, n - 1, cap=nf - 1)[0])]
    run.reset()
    run.begin(first)
    run.kill(n - 1)
    rcs.append(("S>E", eng.scan(first, 5, 4)[0]))
    rcs.append(("E>=n", eng.scan(first, 0, n)[0]))
    rcs.append(("centre>=n", eng.scan(n, 0, n - 1)[0]))
    if fused:
        rcs.append(("part>=nparts", eng.scan_part(first, 0, n - 1, 2, 2)[0]))
        rcs.append(("nparts=0", eng.scan_part(first, 0, n - 1, 0, 0)[0]))
        rcs.append(("part S>E", eng.scan_part(first, 9, 2, 0, 2)[0]))
        rcs.append(("commit dead", eng.scan_commit(np.array([n - 1], np.uint32))[0]))
        rcs.append(("commit descending", eng.scan_commit(np.array([7, 4], np.uint32))[0]))
        rcs.append(("commit twice", eng.scan_commit(np.array([4, 4], np.uint32))[0]))
        rcs.append(("commit range", eng.scan_commit(np.array([n], np.uint32))[0]))
    run.rec("errors", rcs=tuple(rcs))
    run.scan(first, 0, n - 1)  # nothing of the above changed the state
    return run


def diff(a, b):
    """None if the traces are equal, else a description of the first difference."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            if x[0] == y[0]:
                keys = [k for k in x[1] if x[1].get(k) != y[1].get(k)]
                return "record %d (%s): %s" % (i, x[0], {k: (str(x[1].get(k))[:200], str(y[1].get(k))[:200]) for k in keys})
            return "record %d: %s vs %s" % (i, x[0], y[0])
    return None if len(a) == len(b) else "lengths %d vs %d" % (len(a), len(b))
