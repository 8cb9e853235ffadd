"""Host restatement of the flexible GMRES contract (DESIGN.md "Krylov"), the yardstick of
tests/test_krylov_cpu.py and tests/test_gpu_krylov.py.

Restarted FGMRES, right-preconditioned by refsolve.vcycle, classical Gram-Schmidt applied
twice.  Every dot is refsolve.seq_sum of the rounded products (left to right from +0), every
product with A is refsolve.apply_M, every vector update one numpy multiply followed by one
numpy add or subtract (no FMA), every host scalar a Python float operation in the order the
contract writes it -- so the library's ordered path reproduces x, the counts, the norms and
the residual history bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import refsolve


def seq_dot(a, b):
    return refsolve.seq_sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def fgmres(h, b, rtol=1e-8, atol=0.0, restart=30, maxit=100, x0=None, dot=seq_dot):
    """A x = b with A = h.levels[0].A.  Returns a dict: x, rc (0 converged, 1 maxit), its,
    restarts, cycles, converged, bnorm, r0, resid, hist (the estimate after every inner
    iteration)."""
    A = h.levels[0].A
    null = bool(h.nullspace)
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    m = int(restart)
    bnorm = math.sqrt(dot(b, b))
    if x0 is None:
        x = np.zeros(n)
        r = b.copy()
        beta = bnorm
    else:
        x = np.array(x0, dtype=np.float64)
        r = refsolve.apply_M(A, x, 1.0, b, -1.0)
        beta = math.sqrt(dot(r, r))
    target = max(rtol * bnorm, atol)
    out = dict(x=x, rc=0, its=0, restarts=0, cycles=0, converged=0, bnorm=bnorm, r0=beta, resid=beta, hist=[])
    if beta <= target:
        out["converged"] = 1
        return out
    while True:
        V = [r / beta]
        Z = []
        H = {}
        c, s, g = [0.0] * (m + 1), [0.0] * (m + 1), [0.0] * (m + 2)
        g[0] = beta
        j = 0
        while True:
            Z.append(refsolve.vcycle(h, V[j], remove_mean=null))
            out["cycles"] += 1
            w = refsolve.apply_M(A, Z[j])
            col = [0.0] * (j + 2)
            d1 = [dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - d1[i] * V[i]
            d2 = [dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - d2[i] * V[i]
            for i in range(j + 1):
                col[i] = d1[i] + d2[i]
            hn = math.sqrt(dot(w, w))
            col[j + 1] = hn
            with np.errstate(all="ignore"):
                V.append(w / hn)
            out["its"] += 1
            for i in range(j):
                t = c[i] * col[i] + s[i] * col[i + 1]
                col[i + 1] = -s[i] * col[i] + c[i] * col[i + 1]
                col[i] = t
            d = math.sqrt(col[j] * col[j] + col[j + 1] * col[j + 1])
            c[j] = col[j] / d
            s[j] = col[j + 1] / d
            col[j] = c[j] * col[j] + s[j] * col[j + 1]
            for i in range(j + 1):
                H[i, j] = col[i]
            g[j + 1] = -s[j] * g[j]
            g[j] = c[j] * g[j]
            est = abs(g[j + 1])
            out["hist"].append(est)
            k = j + 1
            if est <= target or k == m or out["its"] == maxit or hn == 0.0:
                break
            j += 1
        y = [0.0] * k
        for i in range(k - 1, -1, -1):
            t = g[i]
            for l in range(i + 1, k):
                t = t - H[i, l] * y[l]
            y[i] = t / H[i, i]
        for i in range(k):
            x = x + y[i] * Z[i]
        r = refsolve.apply_M(A, x, 1.0, b, -1.0)
        beta = math.sqrt(dot(r, r))
        out["resid"] = beta
        out["x"] = x
        if beta <= target:
            out["converged"] = 1
            break
        if out["its"] >= maxit:
            out["rc"] = 1
            break
        out["restarts"] += 1
    return out


def crs_krylov(h, ids, b, x0=None, **kw):
    """fgmres in refsolve.crs_solve's id handling: b of local dofs sharing a global id summed in
    ascending local index from +0, x written to every local dof of that id, id 0 untouched"""
    ids = np.asarray(ids, dtype=np.int64)
    b = np.asarray(b, dtype=np.float64)
    n0 = int(h.levels[0].n)
    g = np.zeros(n0)
    for k in range(len(ids)):
        if ids[k]:
            g[ids[k] - 1] = g[ids[k] - 1] + b[k]
    res = fgmres(h, g, **kw)
    x = np.full(len(ids), np.nan) if x0 is None else np.array(x0, dtype=np.float64)
    live = ids != 0
    x[live] = res["x"][ids[live] - 1]
    res["x"] = x
    return res
