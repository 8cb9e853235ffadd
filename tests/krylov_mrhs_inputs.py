"""Inputs shared by tests/test_krylov_mrhs_cpu.py and tests/test_gpu_krylov_mrhs.py: eight
right-hand sides of one operator whose solves end after different numbers of iterations, so that
the lock-step solver's columns finish, hand their slots on and stand at different inner indices.

  column 0, 7   zero guess                     (the longest solves; two restarts at restart 5)
  column 1      the solution itself            (converged at the start: 0 iterations)
  column 2      one V-cycle of b
  column 3      solution + 1e-4 noise
  column 4      solution + 1e-8 noise
  column 5, 6   the restatement's solution at rtol 1e-3 and 1e-6
"""
import numpy as np

import refkrylov
import refsolve

NCOLS = 8
RTOL = 1e-10
MAXIT = 30
CASES = ["amgdmp", "aniso_12", "sem_e2_N7", "p27_8", "p7_12"]
_CACHE = {}


def inputs(case, h):
    """(XS, B, X0), each (n0, 8), for the hierarchy h of fixture `case`; computed once per case"""
    if case not in _CACHE:
        A = h.levels[0].A
        n = int(h.levels[0].n)
        null = bool(h.nullspace)
        rng = np.random.default_rng(11)
        XS = rng.standard_normal((n, NCOLS))
        if null:
            XS = XS - XS.mean(axis=0)
        B = np.stack([refsolve.csr_matvec(A, XS[:, j]) for j in range(NCOLS)], axis=1)
        noise = rng.standard_normal((n, 2))
        X0 = np.zeros((n, NCOLS))
        X0[:, 1] = XS[:, 1]
        X0[:, 2] = refsolve.vcycle(h, B[:, 2], remove_mean=null)
        X0[:, 3] = XS[:, 3] + 1e-4 * noise[:, 0]
        X0[:, 4] = XS[:, 4] + 1e-8 * noise[:, 1]
        X0[:, 5] = refkrylov.fgmres(h, B[:, 5], rtol=1e-3, restart=30, maxit=MAXIT)["x"]
        X0[:, 6] = refkrylov.fgmres(h, B[:, 6], rtol=1e-6, restart=30, maxit=MAXIT)["x"]
        _CACHE[case] = (XS, B, X0)
    return _CACHE[case]


_REF = {}


def reference(case, h, restart, guess):
    """the restatement's run of every column (ordered dots), computed once and shared"""
    key = (case, restart, guess)
    if key not in _REF:
        _, B, X0 = inputs(case, h)
        _REF[key] = [refkrylov.fgmres(h, B[:, j], rtol=RTOL, restart=restart, maxit=MAXIT,
                                      x0=X0[:, j] if guess else None) for j in range(NCOLS)]
    return _REF[key]
