"""Inputs of the Q application and interp_lmop tests (tests/test_gpu_weights.py), built without
a GPU and checked by tests/test_weights_cases_cpu.py, with the oracle's interp and interp_lmop
(oracle/amg_oracle.c: oracle_interp, oracle_interp_lmop) as their reference.  Every builder
asserts the property its case exists for: which support sizes meet which kernel edge, which S
rows fall into which row-pull bin, where the QQ^t chunks split, where the dirty column's walk
lands, which stored entry a hole case lacks.

The matrix is the 27-point Laplacian on 22^3 points (10 648 rows): strictly diagonally dominant,
so every principal submatrix is SPD and every sqrt of the Q factor is of a positive number.
Supports are sorted subsets of its rows."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from omp_amg_amd import problems
from omp_amg_amd.abi import Csr

M = 22
NF = M ** 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "build", "liboracle.so")

QQ_SMALL, QQ_TS = 64, 32                 # amgd_lmop.hip: one-wavefront QQ^t up to 64 points, 32-tiles above
PULL_SMALL, PULL_WAVE, PULL_WIN = 32, 1024, 4096     # S row lengths: thread / wavefront / 4096-wide windows
QQ_BUDGET_MIN = 1 << 20


@functools.lru_cache(maxsize=None)
def matrix():
    Ai, Aj, Av = problems.poisson3d(M, 27)
    ro, col, a = problems.coo_to_csr_np(Ai, Aj, Av)
    assert len(ro) == NF + 1
    return Csr(NF, NF, ro, col, a)


def rows_csr(lists, cn, vals=None):
    """a Csr whose row r holds the sorted columns lists[r] (values vals[r], default 1)"""
    ro = np.zeros(len(lists) + 1, dtype=np.int64)
    for r, l in enumerate(lists):
        l = np.asarray(l, dtype=np.int64)
        assert (np.diff(l) > 0).all() and (len(l) == 0 or (l[0] >= 0 and l[-1] < cn))
        ro[r + 1] = ro[r] + len(l)
    col = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists] + [np.zeros(0, dtype=np.int64)])
    a = np.ones(len(col)) if vals is None else \
        np.concatenate([np.asarray(v, dtype=np.float64) for v in vals] + [np.zeros(0)])
    assert len(a) == len(col)
    return Csr(len(lists), cn, ro, col, a)


def transpose(A):
    """A' with each row's entries in ascending column (= A's row) order"""
    row = np.repeat(np.arange(A.rn), np.diff(A.row_off))
    o = np.lexsort((row, A.col))
    ro = np.zeros(A.cn + 1, dtype=np.int64)
    np.add.at(ro, A.col + 1, 1)
    return Csr(A.cn, A.rn, np.cumsum(ro), row[o], np.asarray(A.a)[o])


def row(A, r):
    return A.col[A.row_off[r]:A.row_off[r + 1]]


def sub_dense(A, P):
    """A restricted to the points P, dense"""
    P = np.asarray(P, dtype=np.int64)
    pos = np.full(A.cn, -1, dtype=np.int64)
    pos[P] = np.arange(len(P))
    D = np.zeros((len(P), len(P)))
    for k, i in enumerate(P.tolist()):
        c = A.col[A.row_off[i]:A.row_off[i + 1]]
        m = pos[c] >= 0
        D[k, pos[c[m]]] = A.a[A.row_off[i]:A.row_off[i + 1]][m]
    return D


def components(A, P):
    """number of connected components of A's graph on the points P"""
    P = np.asarray(P, dtype=np.int64)
    pos = np.full(A.cn, -1, dtype=np.int64)
    pos[P] = np.arange(len(P))
    par = list(range(len(P)))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for k, i in enumerate(P.tolist()):
        for q in pos[A.col[A.row_off[i]:A.row_off[i + 1]]].tolist():
            if q >= 0:
                a, b = find(k), find(q)
                if a != b:
                    par[a] = b
    return len({find(k) for k in range(len(P))})


# ------------------------------------------------------------------ Q application
class QaCase:
    """Wt (supports as rows), Bt (one row per support), u (per support), lam (per point);
    roles: which support carries which special Bt row"""
    def __init__(self, name, supports, seed):
        rng = np.random.default_rng(seed)
        self.name, self.A = name, matrix()
        self.supports = [np.asarray(s, dtype=np.int64) for s in supports]
        nc = len(supports)
        self.sizes = np.array([len(s) for s in supports])
        self.Wt = rows_csr(self.supports, NF)
        self.u = rng.standard_normal(nc)
        self.lam = rng.standard_normal(NF)
        self.roles = {}

    def pick(self, role, ok):
        """the first support not used yet whose size satisfies ok"""
        for c, n in enumerate(self.sizes.tolist()):
            if ok(n) and c not in self.roles.values():
                self.roles[role] = c
                return c
        raise AssertionError(role)

    def finish(self, seed):
        rng = np.random.default_rng(seed)
        r, u, lam = self.roles, self.u, self.lam
        u[r["u_zero"]] = 0.0
        u[r["u_neg"]] = -1.75
        u[r["cancel"]] = 2.0
        pts = np.unique(np.concatenate(self.supports))
        z = rng.choice(pts, size=12, replace=False)
        lam[z[:6]] = 0.0
        lam[z[6:]] = -0.0
        kc = len(self.supports[r["cancel"]]) // 2
        jc = int(self.supports[r["cancel"]][kc])
        lam[jc] = 1.5                                     # b + u * lam = -3 + 2 * 1.5
        cols, vals = [], []
        for c, P in enumerate(self.supports):
            inside = P[rng.random(len(P)) < 0.5]
            outside = np.setdiff1d(rng.choice(NF, size=3, replace=False), P)
            if c == r["empty"]:
                cc = np.zeros(0, dtype=np.int64)
            elif c == r["outside"]:
                cc = np.setdiff1d(rng.choice(NF, size=9, replace=False), P)
            elif c == r["whole"]:
                cc = P.copy()
            elif c == r["around"]:
                cc = np.union1d(inside, [P[0] - 1, P[-1] + 1])
            elif c in (r["negzero"], r["cancel"]):
                cc = np.union1d(inside, [P[len(P) // 2]])
            else:
                cc = np.union1d(inside, outside)
            vv = rng.standard_normal(len(cc))
            if c == r["negzero"]:
                vv[np.searchsorted(cc, P[len(P) // 2])] = -0.0
            if c == r["cancel"]:
                vv[np.searchsorted(cc, jc)] = -3.0
            cols.append(cc)
            vals.append(vv)
        self.Bt = rows_csr(cols, NF, vals)
        # the properties
        B = lambda role: row(self.Bt, r[role])
        P = lambda role: self.supports[r[role]]
        assert len(B("empty")) == 0 and len(P("empty")) > 0
        assert len(B("outside")) > 0 and len(np.intersect1d(B("outside"), P("outside"))) == 0
        assert np.array_equal(B("whole"), P("whole"))
        assert B("around")[0] < P("around")[0] and B("around")[-1] > P("around")[-1]
        assert len(np.intersect1d(B("around"), P("around"))) > 0
        nzv = self.Bt.a[self.Bt.row_off[r["negzero"]]:self.Bt.row_off[r["negzero"] + 1]]
        k = np.nonzero((nzv == 0.0) & np.signbit(nzv))[0]
        assert len(k) == 1 and B("negzero")[k[0]] in P("negzero")
        bv = self.Bt.a[self.Bt.row_off[r["cancel"]]:self.Bt.row_off[r["cancel"] + 1]]
        b = bv[np.searchsorted(B("cancel"), jc)]
        assert jc in P("cancel") and b + u[r["cancel"]] * lam[jc] == 0.0
        assert (u == 0.0).sum() == 1 and (u < 0).sum() >= 1
        lz = lam[pts][lam[pts] == 0.0]
        assert np.signbit(lz).any() and (~np.signbit(lz)).any()
        return self


def _window_support(rng, nz):
    if nz == 0:
        return np.zeros(0, dtype=np.int64)
    lo = int(rng.integers(1, NF - 3 * nz - 1))
    return np.sort(rng.choice(np.arange(lo, lo + 3 * nz), size=nz, replace=False))


TIER_SIZES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512,
              513, 600, 1025, 1400)


@functools.lru_cache(maxsize=None)
def qa_tiers():
    """one support per size around every kernel edge: the 16 / 32-lane groups, a partial 64-row
    group and partial 16 / 32-column tiles of k_qapply_t, LDS against global scratch (512 / 513),
    two supports for the grid-wide kernels at a lowered threshold"""
    rng = np.random.default_rng(101)
    c = QaCase("tiers", [_window_support(rng, nz) for nz in TIER_SIZES], 102)
    assert sorted(c.sizes.tolist()) == sorted(TIER_SIZES)
    c.pick("empty", lambda n: n == 17)
    c.pick("outside", lambda n: n == 65)
    c.pick("whole", lambda n: n == 513)
    c.pick("around", lambda n: n == 15)
    c.pick("negzero", lambda n: n == 257)
    c.pick("cancel", lambda n: n == 600)
    c.pick("u_zero", lambda n: n == 31)
    c.pick("u_neg", lambda n: n == 129)
    return c.finish(103)


@functools.lru_cache(maxsize=None)
def qa_many_small():
    """37 supports of <= 16 points (16 lane groups per block: the third block has 5), 13 of
    17..32 (8 per block: the second has 5) and 5 of 40, in mixed order: both k_split_small passes
    leave a rest"""
    rng = np.random.default_rng(111)
    sizes = [1, 16, 16, 9] + rng.integers(1, 17, size=33).tolist() \
        + [17, 32, 32, 25] + rng.integers(17, 33, size=9).tolist() + [40] * 5
    sizes = np.array(sizes)[rng.permutation(len(sizes))]
    c = QaCase("many_small", [_window_support(rng, int(nz)) for nz in sizes], 112)
    n16, n32, rest = (c.sizes <= 16).sum(), ((c.sizes > 16) & (c.sizes <= 32)).sum(), (c.sizes > 32).sum()
    assert (n16, n32, rest) == (37, 13, 5) and n16 % 16 and n32 % 8
    assert (c.sizes > 16).sum() > 0 and rest > 0              # the rests of the two split passes
    assert len(set(np.sign(np.diff((c.sizes > 16).astype(int))).tolist())) == 3     # mixed order
    c.pick("empty", lambda n: 17 <= n <= 32)
    c.pick("outside", lambda n: n == 40)
    c.pick("whole", lambda n: n == 16)
    c.pick("around", lambda n: 17 <= n <= 32)
    c.pick("negzero", lambda n: n == 40)
    c.pick("cancel", lambda n: 8 <= n <= 16)
    c.pick("u_zero", lambda n: 17 <= n <= 32)
    c.pick("u_neg", lambda n: n <= 16)
    return c.finish(113)


def qa_cases():
    return [qa_tiers(), qa_many_small()]


# ------------------------------------------------------------------ interp_lmop
class LmopCase:
    """W_skel (nf x nc) from its columns' supports: supports[c] the points of column c,
    zeros[c] those of them stored with value 0 (the dirty entries).  S's pattern is
    pattern(Wn Wn'), Wn = W_skel without its zero entries."""
    def __init__(self, name, supports, u, zeros=None, budget=-1):
        self.name, self.A, self.budget = name, matrix(), budget
        self.supports = [np.asarray(s, dtype=np.int64) for s in supports]
        self.nc = len(supports)
        zeros = zeros or {}
        vals = [np.where(np.isin(s, zeros.get(c, [])), 0.0, 1.0) for c, s in enumerate(self.supports)]
        self.Wt = rows_csr(self.supports, NF, vals)
        self.Wskel = transpose(self.Wt)
        self.members = [s[v != 0.0] for s, v in zip(self.supports, vals)]
        self.dirty = np.array([bool((v == 0.0).any()) for v in vals])
        self.sizes = np.array([len(s) for s in self.supports])
        self.u = np.asarray(u, dtype=np.float64)
        assert len(self.u) == self.nc
        self.S = self._pattern()
        self.slen = np.diff(self.S.row_off)

    def _pattern(self):
        of = [[] for _ in range(NF)]
        for c, m in enumerate(self.members):
            for i in m.tolist():
                of[i].append(c)
        self.cols_of = of
        cache, rows = {}, []
        for i in range(NF):
            key = tuple(of[i])
            if key not in cache:
                cache[key] = np.unique(np.concatenate([self.members[c] for c in key])) if key \
                    else np.zeros(0, dtype=np.int64)
            rows.append(cache[key])
        ro = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        col = np.concatenate(rows)
        return Csr(NF, NF, ro, col, np.zeros(len(col)))

    def with_hole(self, name, i, p):
        """the same case with the stored entry at position p of S row i removed"""
        h = object.__new__(LmopCase)
        h.__dict__.update(self.__dict__)
        h.name = name
        k = int(self.S.row_off[i]) + p
        assert 0 <= p < self.slen[i]
        ro = self.S.row_off.copy()
        ro[i + 1:] -= 1
        h.S = Csr(NF, NF, ro, np.delete(self.S.col, k), np.zeros(self.S.nnz - 1))
        h.slen = np.diff(ro)
        h.hole = (i, p, int(self.S.col[k]))
        return h

    def chunks(self):
        """the coarse ranges amgd_lmop forms QQ^t for at a time under this case's budget"""
        budget = max(self.budget if self.budget >= 0 else 16 << 30, QQ_BUDGET_MIN) // 8
        sz = np.where(self.dirty, 0, self.sizes.astype(np.int64) ** 2)
        hsz = np.concatenate([[0], np.cumsum(sz)])
        dend = int(np.nonzero(self.dirty)[0].max()) + 1 if self.dirty.any() else 0
        out, ca = [], dend
        while ca < self.nc:
            cb = ca + 1
            while cb < self.nc and hsz[cb + 1] - hsz[ca] <= budget:
                cb += 1
            if hsz[cb] - hsz[ca]:
                out.append((ca, cb))
            ca = cb
        return out

    def general_only(self):
        """amgd_lmop's test for the general walk: no clean column, or a dirty one after a clean one"""
        clean = np.nonzero(~self.dirty & (self.sizes > 0))[0]
        d = np.nonzero(self.dirty)[0]
        return len(clean) == 0 or (len(d) > 0 and d.max() > clean.min())

    def walk(self, c):
        """sp_add's forward walk (amg_setup.c:1665) of column c over S's global arrays, as
        interp_lmop runs it: for every point k of the support with a non-empty S row, the
        landing of each support column.  Returns the landings (k, m, row walked from, row landed
        in, position), the number past the starting row's end, and the walks that ran off S."""
        S, Q = self.S, self.supports[c]
        rmax = np.where(self.slen > 0, S.col[np.maximum(S.row_off[1:] - 1, 0)], -1)
        lands, offrow, over = [], 0, 0
        for k, j in enumerate(Q.tolist()):
            t, r = int(S.row_off[j]), j
            if self.slen[j] == 0:
                continue
            for m, x in enumerate(Q.tolist()):
                end = int(S.row_off[r + 1])
                if t < end and rmax[r] >= x:
                    r2 = r
                    t = t + int(np.searchsorted(S.col[t:end], x))
                else:
                    nxt = np.nonzero(rmax[r + 1:] >= x)[0]
                    if len(nxt) == 0:
                        over += 1
                        break
                    r2 = r + 1 + int(nxt[0])
                    t = int(S.row_off[r2]) + int(np.searchsorted(row(S, r2), x))
                lands.append((k, m, r, r2, t))
                offrow += t >= S.row_off[j + 1]
                r, t = r2, t + 1
        return lands, offrow, over


def _bins(case):
    L = case.slen
    return {"thr": int(((L > 0) & (L <= PULL_SMALL)).sum()), "wave": int(((L > PULL_SMALL) & (L <= PULL_WAVE)).sum()),
            "blk1": int(((L > PULL_WAVE) & (L <= PULL_WIN)).sum()), "blk2": int((L > PULL_WIN).sum())}


BIN_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 100)


@functools.lru_cache(maxsize=None)
def lmop_clean_bins(budget=-1):
    """every value 1.  Supports around the one-wavefront / tiled QQ^t edge (64 / 65) and partial
    32-tiles; six supports of 700 own + 8 shared points (the shared points' S rows hold 4208
    entries: two windows of the block kernel), one of 1100 (one window); a chain of overlapping
    20-point supports (S rows of exactly 32 and 33 entries, from two supports each); unsupported
    points (empty W_skel and S rows).  The columns are ordered so that the big supports, a chunk
    of QQ^t each under a 1 MB budget, separate neighbours of the chain."""
    rng = np.random.default_rng(201)
    small, base = [], 7
    for nz in BIN_SIZES:
        w = max(2 * nz, 4)
        small.append(np.sort(rng.choice(np.arange(base, base + w), size=nz, replace=False)))
        base += w + 5
    assert base < 1600
    chain, s, q = [], 1600, 0
    steps = (12, 24, 13, 24, 7, 7, 26)
    while s + 20 <= 2900:
        chain.append(np.arange(s, s + 20))
        s += steps[q % len(steps)]
        q += 1
    # the shared points: grid neighbours of the region's first point, of its last and of the one
    # at position 4096, so that the entries the hole cases remove carry a real contribution
    shared = np.array([3001, 3500, 4000, 5000, 6000, 7095, 7097, 7206])
    region = rng.permutation(np.setdiff1d(np.arange(3000, 3000 + 6 * 700 + 8), shared))
    big = [np.sort(np.concatenate([shared, region[700 * g:700 * (g + 1)]])) for g in range(6)]
    one = np.sort(rng.choice(np.arange(7300, 9400), size=1100, replace=False))
    supports = list(small)
    per = (len(chain) + 6) // 7
    for g in range(7):
        supports += chain[g * per:(g + 1) * per]
        if g < 6:
            supports.append(big[g])
    supports.append(one)
    u = rng.standard_normal(len(supports))
    c = LmopCase("clean_bins" if budget < 0 else "qq_chunks", supports, u, budget=budget)
    c.shared, c.big_cols = shared, [k for k, s_ in enumerate(supports) if len(s_) == 708]
    # the properties
    assert not c.dirty.any() and not c.general_only()
    assert sorted(c.sizes[c.sizes != 20].tolist()) == sorted(BIN_SIZES + (708,) * 6 + (1100,))
    assert (c.sizes > QQ_SMALL).sum() >= 3 and any(n % QQ_TS for n in c.sizes if n > QQ_SMALL)
    b = _bins(c)
    assert min(b.values()) > 0, b
    assert (c.slen[shared] == 4208).all() and b["blk2"] == 8 and (c.slen[one] == 1100).all()
    two = np.array([len(o) >= 2 for o in c.cols_of])
    assert ((c.slen == 32) & two).any() and ((c.slen == 33) & two).any()
    assert (np.diff(c.Wskel.row_off) == 0).sum() > 1000 and (c.slen == 0).sum() > 1000
    # the last stored entry of S holds the largest column of all: no walk runs off the end
    assert c.S.col[-1] == c.S.col.max() == max(int(s_[-1]) for s_ in supports)
    if budget >= 0:
        ch = c.chunks()
        assert len(ch) >= 3, ch
        chunk_of = np.zeros(c.nc, dtype=np.int64)
        for q, (ca, cb) in enumerate(ch):
            chunk_of[ca:cb] = q
        mixed = [i for i, o in enumerate(c.cols_of) if len(set(chunk_of[o].tolist())) > 1]
        assert any(c.slen[i] <= PULL_SMALL for i in mixed) and any(c.slen[i] > PULL_WIN for i in mixed)
    else:
        assert len(c.chunks()) == 1
    return c


def lmop_qq_chunks():
    return lmop_clean_bins(QQ_BUDGET_MIN)


@functools.lru_cache(maxsize=None)
def _inv_support(k):
    c = lmop_clean_bins()
    return np.linalg.inv(sub_dense(c.A, c.supports[k]))


def _weight(c, i, j):
    """the largest |u_c (A_cc^-1)(i, j)| over the supports holding both points: what S(i, j) gets"""
    w = 0.0
    for k in c.cols_of[i]:
        P = c.supports[k]
        if j in P:
            w = max(w, abs(c.u[k] * _inv_support(k)[np.searchsorted(P, i), np.searchsorted(P, j)]))
    return w


HOLES = ("hole_small", "hole_mid", "hole_big_first", "hole_big_last", "hole_big_4096")


@functools.lru_cache(maxsize=None)
def lmop_hole(name):
    """clean_bins with one stored entry of S removed: from a row of the thread kernel, of the
    wavefront kernel, and the first, the last and the 4097th entry of a two-window row (the
    last is the column between the two windows).  The contribution to the missing entry lands
    on the next stored one, as in the reference; the row pull has to count the miss."""
    c = lmop_clean_bins()
    two = np.array([len(o) >= 2 for o in c.cols_of])
    if name in ("hole_small", "hole_mid"):           # the heaviest off-diagonal entry of the row
        i = int(np.nonzero((c.slen == 32) & two)[0][0]) if name == "hole_small" \
            else int(np.setdiff1d(c.supports[c.big_cols[1]], c.shared)[350])
        p = max((q for q, j in enumerate(row(c.S, i).tolist()) if j != i),
                key=lambda q: _weight(c, i, int(row(c.S, i)[q])))
    else:
        p = {"hole_big_first": 0, "hole_big_last": 4207, "hole_big_4096": PULL_WIN}[name]
        i = max(c.shared.tolist(), key=lambda q: _weight(c, q, int(row(c.S, q)[p])))
    assert _weight(c, i, int(row(c.S, i)[p])) > 1e-5             # the lost contribution is no zero
    h = c.with_hole(name, i, p)
    L, col = int(h.slen[i]), h.hole[2]
    if name == "hole_small":
        assert 0 < L <= PULL_SMALL
    elif name == "hole_mid":
        assert PULL_SMALL < L <= PULL_WAVE
    else:
        assert L > PULL_WIN
        r = row(h.S, i)
        if name == "hole_big_first":
            assert col < r[0]
        elif name == "hole_big_last":
            assert col > r[-1]
        else:
            assert r[PULL_WIN - 1] < col < r[PULL_WIN]          # between the two windows
    assert any(col in c.supports[k] for k in c.cols_of[i])       # a contribution lands there
    assert h.S.col[-1] == h.S.col.max() and i != NF - 1 and col < h.S.col[-1]
    return h


@functools.lru_cache(maxsize=None)
def lmop_dirty_prefix():
    """column 0: 40 members (value 1) and 300 orphans (value 0) on the lattice of even grid
    coordinates, so mutually uncoupled: isolated points of the support's factor graph.  Orphans
    in the gaps hold only the zero entry (empty S row); orphans inside a later clean support have
    an S row without the pairs.  Clean supports: 24 rows every 200 below row 3000, 50 rows
    each over [8300, 10648): rows [3000, 8300) are empty, so a walk that leaves the low rows skips
    the whole aligned block [4096, 8192)."""
    rng = np.random.default_rng(301)
    idx = np.arange(3000)
    even = idx[(idx % M % 2 == 0) & (idx // M % M % 2 == 0) & (idx // (M * M) % 2 == 0)]
    members = np.arange(1000, 1040)
    even = np.setdiff1d(even, members)
    low = [np.arange(s, s + 24) for s in range(100, 2900, 200)]
    fixed = np.union1d(even[even > 2724], np.intersect1d(even, np.concatenate(low)))
    orphans = np.union1d(fixed, rng.choice(np.setdiff1d(even, fixed), size=300 - len(fixed), replace=False))
    high = [np.arange(s, min(s + 50, NF)) for s in range(8300, NF, 50)]
    supports = [np.union1d(members, orphans)] + low + high
    u = rng.standard_normal(len(supports))
    c = LmopCase("dirty_prefix", supports, u, zeros={0: orphans})
    c.orphans, c.members0 = orphans, members
    # the properties
    assert len(members) == 40 and len(orphans) == 300 and c.sizes[0] >= 64
    assert c.dirty[0] and not c.dirty[1:].any() and not c.general_only()
    A = matrix()
    assert components(A, supports[0]) >= 100                # many isolated points
    assert np.abs(sub_dense(A, orphans) - 26.0 * np.eye(300)).max() == 0.0
    inclean = np.array([len(c.cols_of[i]) > 0 for i in orphans])
    assert (c.slen[orphans[~inclean]] == 0).all() and (~inclean).sum() > 50
    assert inclean.sum() > 20
    for i in orphans[inclean]:
        assert c.slen[i] > 0 and len(np.intersect1d(row(c.S, i), supports[0])) < len(supports[0])
    pts = np.unique(np.concatenate(supports))
    assert ((pts < 3000) | (pts >= 8300)).all() and pts[-1] == NF - 1
    assert c.S.col[-1] == NF - 1
    lands, offrow, over = c.walk(0)
    c.offrow0 = offrow
    assert over == 0 and offrow > 0
    step = [(r, r2) for (_, _, r, r2, _) in lands if r2 != r]
    assert any(r2 == r + 1 for r, r2 in step)                                      # the following row
    assert any(r2 >> 6 > r >> 6 and r2 >> 12 == r >> 12 and r2 > r + 64 for r, r2 in step)   # over 64-row maxima
    assert any((r2 >> 12) - (r >> 12) >= 2 for r, r2 in step)                      # a whole 4096 block
    return c


@functools.lru_cache(maxsize=None)
def lmop_dirty_after_clean():
    """a zero-valued entry in column 2, above the clean columns 0 and 1: the order argument of
    the dirty prefix does not hold and the whole operator takes the general walk"""
    rng = np.random.default_rng(401)
    supports = [np.arange(200, 230), np.arange(260, 300),
                np.union1d(np.arange(400, 420), [225, 350, 430]),
                np.arange(500, 540), np.arange(NF - 48, NF)]
    c = LmopCase("dirty_after_clean", supports, rng.standard_normal(5), zeros={2: [225, 350, 430]})
    assert c.dirty.tolist() == [False, False, True, False, False] and c.general_only()
    assert c.slen[350] == 0 and c.slen[430] == 0 and c.slen[225] == 30
    lands, offrow, over = c.walk(2)
    assert over == 0 and offrow > 0 and c.S.col[-1] == NF - 1
    return c


def lmop_cases():
    """every interp_lmop case (qq_chunks: clean_bins' operands under a 1 MB budget)"""
    return [lmop_clean_bins(), lmop_qq_chunks(), lmop_dirty_prefix(), lmop_dirty_after_clean()] \
        + [lmop_hole(n) for n in HOLES]


# ------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def _oracle():
    if not os.path.exists(ORACLE_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "all"], check=True)
    return C.CDLL(ORACLE_SO)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a if len(a) else np.zeros(1, dtype=np.uint32)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if len(a) else np.zeros(1)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _oracle_interp(name):
    c = {q.name: q for q in qa_cases()}[name]
    A, Wt, Bt = c.A, c.Wt, c.Bt
    keep = [_u64(Wt.row_off), _u32(Wt.col), np.full(Wt.nnz + 1, np.nan), _u64(A.row_off), _u32(A.col),
            _f64(A.a), _u64(Bt.row_off), _u32(Bt.col), _f64(Bt.a), _f64(c.u), _f64(c.lam)]
    _oracle().oracle_interp(C.c_uint32(Wt.rn), C.c_uint32(Wt.cn), *[_p(a) for a in keep])
    out = keep[2][:-1]
    out.setflags(write=False)
    return out


def oracle_interp(case):
    """interp's values on Wt's pattern (computed once per case, read-only)"""
    return _oracle_interp(case.name)


@functools.lru_cache(maxsize=None)
def _oracle_lmop(name):
    name = "clean_bins" if name == "qq_chunks" else name       # the same operands
    c = {q.name: q for q in lmop_cases()}[name]
    A, S, Wt = c.A, c.S, c.Wt
    sa = np.full(S.nnz + 1, np.nan)
    counts = np.zeros(2, dtype=np.uint64)
    keep = [_u64(S.row_off), _u32(S.col), sa, _u64(A.row_off), _u32(A.col), _f64(A.a), _f64(c.u)]
    tk = [_u64(Wt.row_off), _u32(Wt.col)]
    _oracle().oracle_interp_lmop(C.c_uint32(NF), *[_p(a) for a in keep], C.c_uint32(c.nc),
                                 *[_p(a) for a in tk], _p(counts))
    out = sa[:-1]
    out.setflags(write=False)
    return out, int(counts[0]), int(counts[1])


def oracle_lmop(case):
    """(interp_lmop's values on S's pattern, sp_add landings past their row, walks off the end
    of S), computed once per case, read-only"""
    return _oracle_lmop(case.name)
