"""CPU checks of the V-cycle's yardstick (tests/refsolve.py) and of the library's solve
interface: the restatement's products against the reference's own apply_M / apply_Mt, its
contraction on every small fixture, crs_solve's id handling, and the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, REF_SO, golden_cases
from omp_amg_amd import abi, parity
import refsolve


def _hier(case):
    return parity.from_npz(np.load(os.path.join(GOLD, case + ".npz")))


def _csr_mat(M):
    """struct csr_mat (amg_tools.h:5-8) with gslib's 8-byte uint, and the arrays it points into"""
    ro = np.ascontiguousarray(M.row_off, dtype=np.uint64)
    col = np.ascontiguousarray(M.col if M.nnz else np.zeros(1), dtype=np.uint64)
    a = np.ascontiguousarray(M.a if M.nnz else np.zeros(1), dtype=np.float64)
    m = abi.CsrMat(M.rn, M.cn, ro.ctypes.data_as(C.POINTER(abi.amg_uint)),
                   col.ctypes.data_as(C.POINTER(abi.amg_uint)), a.ctypes.data_as(C.POINTER(C.c_double)))
    return m, (ro, col, a)


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64),
                          np.asarray(y, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("case", ["amgdmp", "aniso_12", "p27_8"])
def test_products_match_reference_apply_M(case):
    """refsolve.apply_M / apply_Mt against the reference's own exported routines
    (amg_tools.c:77-115) on W, AfP and Af of every level: bit for bit"""
    if not os.path.exists(REF_SO):
        pytest.skip("reference build not available")
    ref = C.CDLL(REF_SO)
    ref.apply_M.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.POINTER(abi.CsrMat), C.c_void_p]
    ref.apply_M.restype = C.c_double
    ref.apply_Mt.argtypes = [C.c_void_p, C.POINTER(abi.CsrMat), C.c_void_p]
    ref.apply_Mt.restype = C.c_double
    h = _hier(case)
    rng = np.random.default_rng(3)
    for lev in h.levels[:-1]:
        for M in (lev.W, lev.AfP, lev.Af):
            m, keep = _csr_mat(M)
            x, y = rng.standard_normal(M.cn), rng.standard_normal(M.rn)
            z = np.zeros(max(M.rn, 1))
            ref.apply_M(z.ctypes.data, 0.0, None, 1.0, C.byref(m), x.ctypes.data)
            assert _same_bits(z[:M.rn], refsolve.apply_M(M, x))
            ref.apply_M(z.ctypes.data, 1.0, y.ctypes.data, -1.0, C.byref(m), x.ctypes.data)
            assert _same_bits(z[:M.rn], refsolve.apply_M(M, x, 1.0, y, -1.0))
            zt = np.zeros(max(M.cn, 1))
            ref.apply_Mt(zt.ctypes.data, C.byref(m), y.ctypes.data)
            assert _same_bits(zt[:M.cn], refsolve.apply_Mt(M, y))
            del keep


SMALL = [c for c in golden_cases() if int(np.load(os.path.join(GOLD, c + ".npz"))["L0_n"]) <= 2500]


def test_contraction_covers_fixtures():
    assert len(SMALL) >= 20


@pytest.mark.parametrize("case", SMALL)
def test_one_cycle_contracts_in_the_A_norm(case):
    """b = A x*, x* standard normal (seed 1; mean removed on a null space): the A-norm of the
    error after one cycle from x = 0 is below half of its start"""
    h = _hier(case)
    A = h.levels[0].A
    xs = np.random.default_rng(1).standard_normal(A.rn)
    if h.nullspace:
        xs = xs - xs.mean()
    b = refsolve.csr_matvec(A, xs)
    x = refsolve.vcycle(h, b, remove_mean=bool(h.nullspace))
    e0, e1 = xs, xs - x
    n0 = np.sqrt(e0 @ refsolve.csr_matvec(A, e0))
    n1 = np.sqrt(e1 @ refsolve.csr_matvec(A, e1))
    print(f"{case}: A-norm error ratio after one cycle {n1 / n0:.4f}")
    assert n1 < 0.5 * n0, (case, n1 / n0)


def test_crs_id_handling():
    """duplicated dofs are summed in ascending local index, id-0 dofs stay untouched, and a
    permutation of the ids permutes the answer"""
    h = _hier("amgdmp")
    n = int(h.levels[0].n)
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n)
    xg = refsolve.vcycle(h, g, remove_mean=True)
    # a permutation
    perm = rng.permutation(n)
    x = refsolve.crs_solve(h, perm + 1, g[perm], 1)
    assert _same_bits(x, xg[perm])
    # dof 3 three times (its b split in three parts, summed in local order), two id-0 dofs
    parts = np.array([0.1, 1e17, -1e17]) + g[3] / 3
    ids = np.concatenate([np.arange(1, n + 1), [0, 4, 4, 0]])
    b = np.concatenate([g, [7.0, parts[1], parts[2], 9.0]])
    b[3] = parts[0]
    g2 = g.copy()
    g2[3] = ((0.0 + parts[0]) + parts[1]) + parts[2]
    x = refsolve.crs_solve(h, ids, b, 1, x0=np.full(len(ids), 42.0))
    want = refsolve.vcycle(h, g2, remove_mean=True)
    assert _same_bits(x[:n], want)
    assert x[n] == 42.0 and x[n + 3] == 42.0
    assert _same_bits(x[[n + 1, n + 2]], want[[3, 3]])


def test_mean_is_removed():
    h = _hier("amgdmp")
    x = refsolve.vcycle(h, np.random.default_rng(2).standard_normal(int(h.levels[0].n)), remove_mean=True)
    assert abs(refsolve.seq_sum(x)) <= len(x) * np.finfo(float).eps * np.abs(x).sum()


def test_library_exports_the_solve():
    import omp_amg_amd as oa
    if not os.path.exists(oa.LIB_PATH):
        oa.build()
    lib = C.CDLL(oa.LIB_PATH)          # loads without a GPU
    for name in ("amgd_solve_device", "amgd_solve_stats", "crs_solve", "crs_stats",
                 "amgd_test_vc_level", "amgd_test_vc_restrict", "amgd_test_knob"):
        assert hasattr(lib, name), name
    lib.amgd_test_knob_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    for switch in (b"vc_fused", b"vc_tail"):      # the cycle's switches, by name in the table
        v, src = C.c_int64(), C.c_int()
        assert lib.amgd_test_knob_get(switch, C.byref(v), C.byref(src)) == 0, switch
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "omp_amg_amd.h")).read()
    assert "amgd_solve_device" in hdr and "amgd_solve_stats" in hdr


def test_solve_rejects_null_hierarchy_without_gpu():
    """-1 for a missing hierarchy, before anything touches the device"""
    import omp_amg_amd as oa
    if not os.path.exists(oa.LIB_PATH):
        oa.build()
    lib = C.CDLL(oa.LIB_PATH)
    lib.amgd_solve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    assert lib.amgd_solve_device(None, None, None, 0) == -1
