"""Host restatements of single reference operations, for the kernel tests.

Each follows the reference function's operation order exactly (so results are
compared bit for bit):  mxm (amg_setup.c:1894), transpose (:2000), mpm (:1684),
mxmpoint (:1807), apply_M (amg_tools.c:76), min_skel (:2198), build_csr (:3612).
Pure Python -- small matrices only.
"""
import numpy as np

from omp_amg_amd.abi import Csr


def rand_csr(rng, rn, cn, density, ints=False, minrow=0):
    ro = [0]
    cols, vals = [], []
    for i in range(rn):
        k = max(minrow, rng.binomial(cn, density))
        c = np.sort(rng.choice(cn, size=min(k, cn), replace=False))
        v = rng.integers(-3, 4, size=len(c)).astype(float) if ints else rng.standard_normal(len(c))
        if ints:
            v[v == 0] = 1.0
        cols.extend(c.tolist())
        vals.extend(v.tolist())
        ro.append(len(cols))
    return Csr(rn, cn, np.array(ro, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals))


def spgemm(A, B):
    ro, cols, vals = [0], [], []
    for i in range(A.rn):
        acc = {}
        s, e = A.row_off[i], A.row_off[i + 1]
        for ka in range(s, e):
            if ka + 1 < e and A.col[ka + 1] == A.col[ka]:
                continue
            k, av = A.col[ka], A.a[ka]
            for kb in range(B.row_off[k], B.row_off[k + 1]):
                j = B.col[kb]
                acc[j] = acc.get(j, 0.0) + B.a[kb] * av
        for j in sorted(acc):
            if acc[j] != 0.0:
                cols.append(j)
                vals.append(acc[j])
        ro.append(len(cols))
    return Csr(A.rn, B.cn, np.array(ro), np.array(cols, dtype=np.int64), np.array(vals))


def transpose(A):
    ent = []
    for i in range(A.rn):
        for k in range(A.row_off[i], A.row_off[i + 1]):
            ent.append((A.col[k], i, A.a[k]))
    ent.sort(key=lambda t: (t[0], t[1]))   # stable
    ro = np.zeros(A.cn + 1, dtype=np.int64)
    for c, _, _ in ent:
        ro[c + 1] += 1
    return Csr(A.cn, A.rn, np.cumsum(ro), np.array([t[1] for t in ent], dtype=np.int64),
               np.array([t[2] for t in ent]))


def mpm(alpha, A, beta, B):
    ro, cols, vals = [0], [], []
    for i in range(A.rn):
        ja, ea, jb, eb = A.row_off[i], A.row_off[i + 1], B.row_off[i], B.row_off[i + 1]
        while ja < ea or jb < eb:
            if ja < ea and jb < eb:
                if A.col[ja] == B.col[jb]:
                    s = alpha * A.a[ja] + beta * B.a[jb]
                    if s != 0.0:
                        cols.append(A.col[ja]); vals.append(s)
                    ja += 1; jb += 1
                elif A.col[ja] < B.col[jb]:
                    cols.append(A.col[ja]); vals.append(alpha * A.a[ja]); ja += 1
                else:
                    cols.append(B.col[jb]); vals.append(beta * B.a[jb]); jb += 1
            elif ja == ea:
                cols.append(B.col[jb]); vals.append(beta * B.a[jb]); jb += 1
            else:
                cols.append(A.col[ja]); vals.append(alpha * A.a[ja]); ja += 1
        ro.append(len(cols))
    return Csr(A.rn, A.cn, np.array(ro), np.array(cols, dtype=np.int64), np.array(vals))


def mxmpoint(A, B):
    ro, cols, vals = [0], [], []
    for i in range(A.rn):
        ja, ea, jb, eb = A.row_off[i], A.row_off[i + 1], B.row_off[i], B.row_off[i + 1]
        while ja < ea and jb < eb:
            if A.col[ja] == B.col[jb]:
                cols.append(A.col[ja]); vals.append(A.a[ja] * B.a[jb]); ja += 1; jb += 1
            elif A.col[ja] < B.col[jb]:
                ja += 1
            else:
                jb += 1
        ro.append(len(cols))
    return Csr(A.rn, A.cn, np.array(ro), np.array(cols, dtype=np.int64), np.array(vals))


def spmv(A, x, alpha=0.0, y=None, beta=1.0):
    z = np.zeros(A.rn)
    for i in range(A.rn):
        t = 0.0
        for k in range(A.row_off[i], A.row_off[i + 1]):
            t += A.a[k] * x[A.col[k]]
        z[i] = beta * t if (alpha == 0.0 or y is None) else alpha * y[i] + beta * t
    return z


def min_skel(R):
    ro = np.arange(R.rn + 1, dtype=np.int64)
    cols, vals = [], []
    for i in range(R.rn):
        ym, j = -np.finfo(float).max, 0
        for k in range(R.row_off[i], R.row_off[i + 1]):
            if R.a[k] > ym:
                ym, j = R.a[k], R.col[k]
        cols.append(j)
        vals.append(1.0 if ym > 0.0 else 0.0)
    return Csr(R.rn, R.cn, ro, np.array(cols, dtype=np.int64), np.array(vals))


def same(X, Y):
    return (X.rn == Y.rn and X.cn == Y.cn and np.array_equal(X.row_off, Y.row_off)
            and np.array_equal(X.col, Y.col)
            and np.array_equal(np.asarray(X.a).view(np.uint64), np.asarray(Y.a).view(np.uint64)))


def expand_pick(X):
    """expand_support's pick per row (amg_setup.c:1000-1115): |X| ranked by descending
    value, ties in column order (glibc qsort, stable); running sum of the nonzero
    values against half the total; the first N = 1 + #{sum - V < 0} ranks (capped at
    the row length) are picked.  Returns the picked pattern as a Csr of ones."""
    ro, cols = [0], []
    for i in range(X.rn):
        s, e = X.row_off[i], X.row_off[i + 1]
        v = np.abs(np.asarray(X.a[s:e]))
        order = sorted(range(e - s), key=lambda q: (-v[q], q))
        sv = [v[q] for q in order]
        tot = 0.0
        for x in sv:
            if x != 0.0:
                tot += x
        V = tot * 0.5
        c = 0
        if V != 0.0:
            run = 0.0
            for x in sv:
                if x != 0.0:
                    run += x
                if run - V < 0:
                    c += 1
        N = min(c + 1, e - s)
        picked = sorted(int(X.col[s + q]) for q in order[:N])
        cols.extend(picked)
        ro.append(len(cols))
    return Csr(X.rn, X.cn, np.array(ro), np.array(cols, dtype=np.int64), np.ones(len(cols)))


# --------------------------------------------------------------------------- find_support
# (amg_setup.c:1260-1407), numpy only.  Sums run left to right from +0 like the reference's
# apply_M / apply_Mt; a removed entry is an exact zero that stays in the pattern.
DBL_MAX = float(np.finfo(float).max)
FSL_CH = 2048                     # amgd_interp.hip: entries per chunk of a long column


def ordered_rowsum(ro, p):
    """per row of the offsets ro, the entries of p added left to right starting from +0"""
    ro = np.asarray(ro, dtype=np.int64)
    ln = np.diff(ro)
    t = np.zeros(len(ln))
    act = np.nonzero((ln > 0) & (ln <= 64))[0]
    base, k = ro[act], 0
    while len(act):
        t[act] += p[base + k]
        k += 1
        keep = ln[act] > k
        act, base = act[keep], base[keep]
    for i in np.nonzero(ln > 64)[0]:
        s = 0.0
        for v in p[ro[i]:ro[i + 1]].tolist():
            s += v
        t[i] = s
    return t


class Csc:
    """R's columns: offsets, row indices, and for every CSC position its CSR position"""
    def __init__(self, R):
        col = np.asarray(R.col, dtype=np.int64)
        self.perm = np.argsort(col, kind="stable")
        self.row = np.repeat(np.arange(R.rn, dtype=np.int64), np.diff(np.asarray(R.row_off, dtype=np.int64)))[self.perm]
        self.ro = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=R.cn))]).astype(np.int64)


def fs_products(R, T, a):
    """rs = R 1, w = R' rs, tmp = R w, w2 = R' tmp on the values a (CSR order)"""
    ro, col = np.asarray(R.row_off, dtype=np.int64), np.asarray(R.col, dtype=np.int64)
    rs = ordered_rowsum(ro, a)
    w = ordered_rowsum(T.ro, a[T.perm] * rs[T.row])
    tmp = ordered_rowsum(ro, a * w[col])
    w2 = ordered_rowsum(T.ro, a[T.perm] * tmp[T.row])
    return rs, w, tmp, w2


def _select_into(T, a, rs, w, sumR, thr, c0=0, c1=None):
    """the selection of one sweep on the CSR values a (changed in place): [(i, c)] by column"""
    c1 = len(T.ro) - 1 if c1 is None else c1
    sel = []
    for c in (np.nonzero((w[c0:c1] > thr) & (sumR[c0:c1] != 0.0))[0] + c0).tolist():
        s, e = T.ro[c], T.ro[c + 1]
        i, best = 0, -1
        if e > s:
            x = a[T.perm[s:e]] * rs[T.row[s:e]]
            m = int(np.argmax(x))                 # the first largest: strict > from -DBL_MAX
            if x[m] > -DBL_MAX:
                best, i = s + m, int(T.row[s + m])
        sel.append((i, c, best))
    for _, _, best in sel:
        if best >= 0:
            a[T.perm[best]] = 0.0
    return sel


def fs_select(R, rs, w, sumR, thr, c0=0, c1=None, windowed=False):
    """one sweep (amg_setup.c:1323-1407): per bad column (w > thr and sumR != 0, columns
    [c0, c1)) the first row of the largest R_ic * rs_i is zeroed, then the rows and columns
    that lost an entry are re-summed left to right from +0.  windowed: the partitioned
    driver's form -- only R' (the window) loses the entries; R, rs and sumR stay.  Returns
    sel (pairs sorted by column), removed (any entry zeroed), Ra, Rta, rs, sumR."""
    T = Csc(R)
    a0 = np.array(R.a, dtype=np.float64)
    a = a0.copy()
    rs, sumR = np.array(rs, dtype=np.float64), np.array(sumR, dtype=np.float64)
    sel = _select_into(T, a, rs, np.asarray(w), sumR, thr, c0, c1)
    removed = any(b >= 0 for _, _, b in sel)
    if not windowed and removed:
        ro = np.asarray(R.row_off, dtype=np.int64)
        for i in sorted({i for i, _, _ in sel}):
            rs[i] = ordered_rowsum(np.array([0, ro[i + 1] - ro[i]]), a[ro[i]:ro[i + 1]])[0]
        for _, c, _ in sel:
            sumR[c] = ordered_rowsum(np.array([0, T.ro[c + 1] - T.ro[c]]), a[T.perm[T.ro[c]:T.ro[c + 1]]])[0]
    pairs = np.array([(i, c) for i, c, _ in sel], dtype=np.int64).reshape(-1, 2)
    return {"sel": pairs, "removed": removed, "Ra": a0 if windowed else a, "Rta": a[T.perm], "rs": rs,
            "sumR": sumR}


def fs_expand(M, rows, stamp, tag):
    """distinct columns of the listed rows of M whose stamp is not tag (sorted), stamps after"""
    ro, col = np.asarray(M.row_off, dtype=np.int64), np.asarray(M.col, dtype=np.int64)
    st = np.array(stamp, dtype=np.uint32)
    nb = set()
    for i in np.unique(np.asarray(rows, dtype=np.int64)).tolist():
        nb.update(col[ro[i]:ro[i + 1]].tolist())
    out = np.array(sorted(c for c in nb if st[c] != tag), dtype=np.int64)
    st[out] = tag
    return out, st


class FsUndefined(Exception):
    """find_support met one of the library's UB() exits (the reference does not terminate)"""


def find_support(R, goal, max_sweeps=100000):
    """the whole loop (amg_setup.c:1260).  Raises FsUndefined where the library takes a UB()
    exit: theta reaches 0 (1), nf <= 1 (2), nothing removed (3), capacity reached (4).
    Returns Sk and a trace: sweeps, the first sweep's products and max(v), per selecting sweep
    the selected pairs, and whether the library's incremental path would serve the sweep
    after it (three expansions within the caps nc/4+1, nf/4+1, nc/4+1)."""
    nf, nc = R.rn, R.cn
    ro, col = np.asarray(R.row_off, dtype=np.int64), np.asarray(R.col, dtype=np.int64)
    T = Csc(R)
    a = np.array(R.a, dtype=np.float64)
    nnz = len(a)
    cap = nnz + nc + 16
    cap_c, cap_r = nc // 4 + 1, nf // 4 + 1
    theta, it, ns = 0.5, 0, 0
    sels, inc_next, first, mv1 = [], [], None, None
    while True:
        it += 1
        if it > max_sweeps:
            raise FsUndefined("no end within max_sweeps")
        rs, w, tmp, w2 = fs_products(R, T, a)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(w == 0.0, 0.0, w2 / w)
        mv = float(v.max()) if nc else -DBL_MAX
        if it == 1:
            first, mv1 = (rs, w, tmp, w2), mv
        if mv < goal:
            break
        while mv <= (1 + theta) * goal and theta > 0:
            theta = theta / 2.0
        if theta == 0:
            raise FsUndefined("UB(1): theta reached 0")
        if nf <= 1:
            raise FsUndefined("UB(2): nf <= 1")
        sumR = ordered_rowsum(T.ro, a[T.perm])
        sel = _select_into(T, a, rs, w, sumR, (1 + theta) * goal)
        if not any(b >= 0 for _, _, b in sel):
            raise FsUndefined("UB(3): nothing removed")
        pairs = np.array([(i, c) for i, c, _ in sel], dtype=np.int64).reshape(-1, 2)
        sels.append(pairs)
        ns += len(sel)
        if ns + nc > cap:
            raise FsUndefined("UB(4): capacity reached")
        ok = len(sel) <= cap_c
        if ok:
            c1 = np.unique(np.concatenate([col[ro[i]:ro[i + 1]] for i in np.unique(pairs[:, 0])]))
            ok = len(c1) <= cap_c
        if ok:
            d2 = np.unique(np.concatenate([T.row[T.ro[c]:T.ro[c + 1]] for c in c1]))
            ok = len(d2) <= cap_r
        if ok:
            c3 = np.unique(np.concatenate([col[ro[i]:ro[i + 1]] for i in d2]))
            ok = len(c3) <= cap_c
        inc_next.append(bool(ok))
    allp = np.concatenate(sels) if sels else np.zeros((0, 2), dtype=np.int64)
    key = allp[:, 0] * max(nc, 1) + allp[:, 1]
    if len(np.unique(key)) != len(key):
        raise FsUndefined("an entry was selected twice")
    order = np.argsort(key, kind="stable")
    sk_ro = np.concatenate([[0], np.cumsum(np.bincount(allp[:, 0], minlength=nf))]).astype(np.int64)
    Sk = Csr(nf, nc, sk_ro, allp[order, 1].copy(), np.ones(len(key)))
    return Sk, {"sweeps": it, "first": first, "mv_first": mv1, "sels": sels, "inc_next": inc_next,
                "col_len": np.diff(T.ro)}
