"""Host restatement of the V-cycle contract (DESIGN.md "Solve"; reference amg.c:114-189,
amg_tools.c:77-115), the yardstick of tests/test_solve_cpu.py and tests/test_gpu_solve.py.

Written per level with the C/F masks of the exported hierarchy -- deliberately NOT in the
library's flat level-ordered layout, so a comparison also checks the library's permutation.
Every row sum is sequential, left to right from +0: the k-th entries of all rows are added in
one vectorised pass (numpy multiplies, then adds -- no FMA), never np.sum.  The transposed
product orders each column's entries by a stable argsort of the column indices, i.e. in
ascending row order, as apply_Mt's scatter visits them.
"""
from __future__ import annotations

import numpy as np


def _seq_rowsum(ro, p):
    """t[i] = ((0 + p[ro[i]]) + p[ro[i]+1]) + ... for every row, k-th entries in one pass"""
    ro = np.asarray(ro, dtype=np.int64)
    rn = len(ro) - 1
    t = np.zeros(rn)
    if rn == 0:
        return t
    lens = ro[1:] - ro[:-1]
    rows = np.nonzero(lens > 0)[0]
    k = 0
    while len(rows):
        t[rows] = t[rows] + p[ro[rows] + k]
        k += 1
        rows = rows[lens[rows] > k]
    return t


def apply_M(M, x, alpha=0.0, y=None, beta=1.0):
    """z = alpha*y + beta*(M x), or beta*(M x) when alpha == 0 or y is None (amg_tools.c:77)"""
    x = np.asarray(x, dtype=np.float64)
    col = np.asarray(M.col, dtype=np.int64)[:M.nnz]
    a = np.asarray(M.a, dtype=np.float64)[:M.nnz]
    t = _seq_rowsum(M.row_off, a * x[col] if M.nnz else np.zeros(0))
    if alpha == 0.0 or y is None:
        return beta * t
    return alpha * np.asarray(y, dtype=np.float64) + beta * t


def apply_Mt(M, x):
    """z = M' x: per column the products a*x[row] in ascending row order from +0 (amg_tools.c:103)"""
    x = np.asarray(x, dtype=np.float64)
    nnz = M.nnz
    col = np.asarray(M.col, dtype=np.int64)[:nnz]
    a = np.asarray(M.a, dtype=np.float64)[:nnz]
    ro = np.asarray(M.row_off, dtype=np.int64)
    row = np.repeat(np.arange(M.rn, dtype=np.int64), ro[1:] - ro[:-1])
    p = a * x[row] if nnz else np.zeros(0)
    order = np.argsort(col, kind="stable")
    tro = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=M.cn))]).astype(np.int64)
    return _seq_rowsum(tro, p[order])


def cheb_scalars(rho, m):
    """(beta, gamma) of every Chebyshev update after the first c, in the reference's operation
    order (amg.c:148-149, :158)"""
    out = []
    if m > 1:
        alpha = rho / 2
        alpha *= alpha
        gamma = 2 * alpha / (1 - 2 * alpha)
        beta = 1 + gamma
        out.append((beta, gamma))
        for _ in range(3, m + 1):
            gamma = alpha * beta
            gamma = gamma / (1 - gamma)
            beta = 1 + gamma
            out.append((beta, gamma))
    return out


def restrict(W, bF, bC):
    """b_{l+1} = 1*b_l[C] + 1*(W' b_l[F]) (amg.c:125-126)"""
    return 1.0 * np.asarray(bC, dtype=np.float64) + 1.0 * apply_Mt(W, bF)


def level_up(Af, W, AfP, D, m, rho, bF, xc):
    """one level of the up-sweep (amg.c:139-166): returns (xf, bf, c) with xf the F part of the
    level's solution, bf = b[F] - AfP xc, c the last Chebyshev iterate"""
    D = np.asarray(D, dtype=np.float64)
    xf = apply_M(W, xc)
    bf = apply_M(AfP, xc, 1.0, bF, -1.0)
    c = D * bf
    c_old = None
    for k, (beta, gamma) in enumerate(cheb_scalars(float(rho), int(m))):
        r = apply_M(Af, c, 1.0, bf, -1.0)
        if k == 0:
            c, c_old = beta * (c + D * r), c
        else:
            c, c_old = beta * (c + D * r) - gamma * c_old, c
    return xf + c, bf, c


def seq_sum(v):
    s = 0.0
    for t in np.asarray(v, dtype=np.float64):
        s = s + float(t)
    return s


def vcycle(h, b, remove_mean=False):
    """x = one V-cycle of the exported hierarchy h (abi.Hierarchy) on b, both in level-0 row
    order.  remove_mean: x -= (1/n) sum(x), the sum left to right in the level-ordered layout
    (F points of level 0, of level 1, ..., the bottom point), amg.c:181-184."""
    nl = h.nlevels
    bs = [np.array(b, dtype=np.float64)]
    for l in range(nl - 1):
        lev = h.levels[l]
        F, Cm = lev.F != 0, lev.C != 0
        bs.append(restrict(lev.W, bs[l][F], bs[l][Cm]))
    a = h.levels[nl - 1].A
    d = 0.0 if h.nullspace != 0 else 1.0 / float(a.a[0])
    x = np.array([d * bs[nl - 1][0]]) if int(h.levels[nl - 1].n) else np.zeros(0)
    flat = [x]
    for l in range(nl - 2, -1, -1):
        lev = h.levels[l]
        F, Cm = lev.F != 0, lev.C != 0
        xf, _, _ = level_up(lev.Af, lev.W, lev.AfP, lev.D, int(lev.m), lev.rho, bs[l][F], x)
        xl = np.zeros(len(F))
        xl[F] = xf
        xl[Cm] = x
        x = xl
        flat.insert(0, xf)
    if remove_mean:
        n = len(x)
        avg = (1.0 / n) * seq_sum(np.concatenate(flat))
        x = x - avg
    return x


def crs_solve(h, ids, b, null_space, x0=None):
    """crs_solve's id handling around the cycle: b of local dofs sharing a global id summed in
    ascending local index from +0, x written to every local dof of that id, id 0 untouched"""
    ids = np.asarray(ids, dtype=np.int64)
    b = np.asarray(b, dtype=np.float64)
    n0 = int(h.levels[0].n)
    g = np.zeros(n0)
    for k in range(len(ids)):
        if ids[k]:
            g[ids[k] - 1] = g[ids[k] - 1] + b[k]
    xg = vcycle(h, g, remove_mean=bool(null_space))
    x = np.full(len(ids), np.nan) if x0 is None else np.array(x0, dtype=np.float64)
    live = ids != 0
    x[live] = xg[ids[live] - 1]
    return x


def csr_matvec(M, x):
    """plain product for norms (order irrelevant)"""
    ro = np.asarray(M.row_off, dtype=np.int64)
    row = np.repeat(np.arange(M.rn), ro[1:] - ro[:-1])
    return np.bincount(row, weights=np.asarray(M.a)[:M.nnz] * np.asarray(x)[np.asarray(M.col)[:M.nnz]],
                       minlength=M.rn)
