"""The flexible GMRES contract on the host (tests/refkrylov.py over tests/refsolve.py), without a
GPU: it converges on the committed fixtures in few iterations, restarts work, the recurrence's
residual estimate is the true residual, the cycle is measurably not symmetric (why the wrapper
is GMRES and not CG), and the public header declares the entry points."""
import os

import numpy as np
import pytest

from conftest import GOLD
from omp_amg_amd import parity
import refkrylov
import refsolve
from test_abi_cpu import declared_functions

CASES = ["p7_12", "aniso_12", "sem_e2_N7", "p27_8", "amgdmp"]
RTOL = 1e-10
_H, _RES = {}, {}


def hier(case):
    if case not in _H:
        _H[case] = parity.from_npz(np.load(os.path.join(GOLD, case + ".npz")))
    return _H[case]


def rhs(h):
    """b = A x*, x* standard normal with the mean removed on a null space"""
    A = h.levels[0].A
    xs = np.random.default_rng(5).standard_normal(int(h.levels[0].n))
    if h.nullspace:
        xs = xs - xs.mean()
    return refsolve.csr_matvec(A, xs)


def solve(case, restart):
    """one restatement run per (case, restart), shared by the tests"""
    if (case, restart) not in _RES:
        h = hier(case)
        b = rhs(h)
        _RES[case, restart] = (b, refkrylov.fgmres(h, b, rtol=RTOL, restart=restart, maxit=20))
    return _RES[case, restart]


@pytest.mark.parametrize("case", CASES)
def test_converges_within_20_iterations(case):
    b, res = solve(case, 30)
    assert res["rc"] == 0 and res["converged"] == 1, res["hist"]
    assert 1 <= res["its"] <= 20 and res["restarts"] == 0 and res["cycles"] == res["its"]
    assert res["resid"] <= RTOL * res["bnorm"]
    assert len(res["hist"]) == res["its"]


@pytest.mark.parametrize("case", CASES)
def test_restart_5_converges_and_restarts(case):
    b, res = solve(case, 5)
    assert res["rc"] == 0 and res["its"] <= 20, res["hist"]
    assert res["restarts"] >= 2


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("restart", [30, 5])
def test_estimate_is_the_true_residual(case, restart):
    """the last estimate of the recurrence against ||b - A x|| recomputed by another route"""
    b, res = solve(case, restart)
    h = hier(case)
    true = np.linalg.norm(b - refsolve.csr_matvec(h.levels[0].A, res["x"]))
    assert abs(res["hist"][-1] - true) <= 1e-3 * true, (res["hist"][-1], true)
    assert abs(res["resid"] - true) <= 1e-3 * true


@pytest.mark.parametrize("case", CASES)
def test_cycle_is_not_symmetric(case):
    """|v'Bu - u'Bv| / (|u| |Bv|) for the cycle B: rounding alone would give about 1e-13"""
    h = hier(case)
    rng = np.random.default_rng(5)
    n = int(h.levels[0].n)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    null = bool(h.nullspace)
    Bu, Bv = refsolve.vcycle(h, u, remove_mean=null), refsolve.vcycle(h, v, remove_mean=null)
    asym = abs(v @ Bu - u @ Bv) / (np.linalg.norm(u) * np.linalg.norm(Bv))
    assert asym > 1e-6, asym


def test_maxit_returns_the_last_iterate():
    b, full = solve("p27_8", 30)
    res = refkrylov.fgmres(hier("p27_8"), b, rtol=RTOL, restart=30, maxit=4)
    assert res["rc"] == 1 and res["its"] == 4 and res["converged"] == 0
    assert res["hist"] == full["hist"][:4]
    assert res["resid"] > RTOL * res["bnorm"]


def test_zero_rhs_and_initial_guess():
    h = hier("p27_8")
    n = int(h.levels[0].n)
    res = refkrylov.fgmres(h, np.zeros(n), rtol=RTOL)
    assert res["rc"] == 0 and res["its"] == 0 and not res["x"].any()
    b, full = solve("p27_8", 30)
    warm = refkrylov.fgmres(h, b, rtol=RTOL, restart=30, maxit=20, x0=refsolve.vcycle(h, b))
    assert warm["rc"] == 0 and warm["its"] <= full["its"] and warm["r0"] < full["r0"]


def test_header_declares_the_krylov_entry_points():
    assert {"amgd_krylov_device", "amgd_krylov_stats", "amgd_crs_krylov"} <= declared_functions()
