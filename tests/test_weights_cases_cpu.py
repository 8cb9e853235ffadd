"""The inputs of the Q application and interp_lmop tests (tests/weights_cases.py) and their
reference, checked without a GPU: every builder's property asserts run; the oracle's exported
interp / interp_lmop (the checkers of tests/test_gpu_weights.py) equal the reference's own
routines bit for bit where the reference build exists; and, independent of any operation
order, they agree with dense solves: interp's row c is A_cc^-1 (b_c + u_c lambda_c), the clean
constraint operator is sum_c u_c P_c A_cc^-1 P_c'."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REF_SO
from omp_amg_amd import abi
import weights_cases as wc

DENSE_MAX = 600                   # supports up to this many points are solved densely

QA = {"tiers": wc.qa_tiers, "many_small": wc.qa_many_small}
LMOP = {"clean_bins": wc.lmop_clean_bins, "qq_chunks": wc.lmop_qq_chunks,
        "dirty_prefix": wc.lmop_dirty_prefix, "dirty_after_clean": wc.lmop_dirty_after_clean}
LMOP.update({n: (lambda n=n: wc.lmop_hole(n)) for n in wc.HOLES})


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(QA))
def test_qa_builder(name):
    """the builder's own asserts, and the oracle writes every entry of Wt's pattern"""
    c = QA[name]()
    out = wc.oracle_interp(c)
    assert len(out) == c.Wt.nnz and np.isfinite(out).all()


@pytest.mark.parametrize("name", list(LMOP))
def test_lmop_builder(name):
    """the builder's own asserts; the oracle's walk never runs off the end of S (past it the
    reference is undefined, so nothing would define the right answer)"""
    c = LMOP[name]()
    sa, offrow, over = wc.oracle_lmop(c)
    assert over == 0
    assert len(sa) == c.S.nnz and np.isfinite(sa).all()
    if name == "dirty_prefix":
        assert offrow == c.offrow0 > 0          # the builder's replay of column 0's walk
    elif name in ("clean_bins", "qq_chunks"):
        assert offrow == 0
    elif name == "dirty_after_clean":
        assert offrow > 0
    else:                                       # the orphaned contribution landed on another entry
        i, p, _ = c.hole
        whole = np.delete(wc.oracle_lmop(wc.lmop_clean_bins())[0], c.S.row_off[i] + p)
        assert not np.array_equal(_bits(whole), _bits(sa))


def _csr_mat(M, a=None):
    """struct csr_mat (amg_tools.h:5-8) with gslib's 8-byte uint, and the arrays it points into"""
    ro = np.ascontiguousarray(M.row_off, dtype=np.uint64)
    col = np.ascontiguousarray(M.col if M.nnz else np.zeros(1), dtype=np.uint64)
    a = np.array(M.a if a is None else a, dtype=np.float64) if M.nnz else np.zeros(1)
    m = abi.CsrMat(M.rn, M.cn, ro.ctypes.data_as(C.POINTER(abi.amg_uint)),
                   col.ctypes.data_as(C.POINTER(abi.amg_uint)), a.ctypes.data_as(C.POINTER(C.c_double)))
    return m, (ro, col, a)


def _ref():
    if not os.path.exists(REF_SO):
        pytest.skip("reference build not available")
    ref = C.CDLL(REF_SO)
    ref.interp.argtypes = [C.POINTER(abi.CsrMat)] * 3 + [C.c_void_p, C.c_void_p]
    ref.interp.restype = None
    ref.interp_lmop.argtypes = [C.POINTER(abi.CsrMat), C.POINTER(abi.CsrMat), C.c_void_p, C.POINTER(abi.CsrMat)]
    ref.interp_lmop.restype = C.c_int
    return ref


@pytest.mark.parametrize("name", list(QA))
def test_oracle_interp_is_the_reference(name):
    """oracle_interp against the reference's own interp (amg_setup.c:2053): bit for bit"""
    ref = _ref()
    c = QA[name]()
    wt, kw = _csr_mat(c.Wt, np.full(c.Wt.nnz, np.nan))
    at, ka = _csr_mat(c.A)
    bt, kb = _csr_mat(c.Bt)
    u, lam = np.array(c.u), np.array(c.lam)
    ref.interp(C.byref(wt), C.byref(at), C.byref(bt), u.ctypes.data, lam.ctypes.data)
    assert np.array_equal(_bits(kw[2]), _bits(wc.oracle_interp(c)))


@pytest.mark.parametrize("name", [n for n in LMOP if n != "qq_chunks"])
def test_oracle_interp_lmop_is_the_reference(name):
    """oracle_interp_lmop against the reference's own interp_lmop (amg_setup.c:1589), off-row
    landings of sp_add included: bit for bit"""
    ref = _ref()
    c = LMOP[name]()
    st, ks = _csr_mat(c.S, np.full(c.S.nnz, np.nan))
    at, ka = _csr_mat(c.A)
    wt, kw = _csr_mat(c.Wt)
    u = np.array(c.u)
    assert ref.interp_lmop(C.byref(st), C.byref(at), u.ctypes.data, C.byref(wt)) == 1
    assert np.array_equal(_bits(ks[2]), _bits(wc.oracle_lmop(c)[0]))


def _inv(c, P):
    return np.linalg.inv(wc.sub_dense(c.A, P))


def _qa_dense_errors(c):
    out, errs = wc.oracle_interp(c), []
    for k, P in enumerate(c.supports):
        if not 0 < len(P) <= DENSE_MAX:
            continue
        b = np.zeros(len(P))
        bc, bv = wc.row(c.Bt, k), c.Bt.a[c.Bt.row_off[k]:c.Bt.row_off[k + 1]]
        m = np.isin(bc, P)
        b[np.searchsorted(P, bc[m])] = bv[m]
        want = np.linalg.solve(wc.sub_dense(c.A, P), b + c.u[k] * c.lam[P])
        got = out[c.Wt.row_off[k]:c.Wt.row_off[k + 1]]
        n = np.linalg.norm(want)
        errs.append(np.linalg.norm(got - want) / n if n else np.linalg.norm(got))
    return np.array(errs)


def _lmop_dense_errors(c):
    """per support of up to DENSE_MAX points whose points lie in such supports only: the block
    of S on the support against the dense sum"""
    sa = wc.oracle_lmop(c)[0]
    small = [k for k in range(c.nc) if 0 < c.sizes[k] <= DENSE_MAX]
    ok = np.zeros(c.nc, dtype=bool)
    ok[small] = True
    small = [k for k in small if all(ok[c.cols_of[i]].all() for i in c.supports[k])]
    n = int(max(c.supports[k][-1] for k in small)) + 1
    Sd, So = np.zeros((n, n)), np.zeros((n, n))
    for k in small:
        P = c.supports[k]
        Sd[np.ix_(P, P)] += c.u[k] * _inv(c, P)
    for i in range(n):
        So[i, wc.row(c.S, i)] = sa[c.S.row_off[i]:c.S.row_off[i + 1]]
    errs = []
    for k in small:
        ix = np.ix_(c.supports[k], c.supports[k])
        errs.append(np.linalg.norm(So[ix] - Sd[ix]) / np.linalg.norm(Sd[ix]))
    return np.array(errs), len(small)


# measured on the CPU (largest per-support relative error of the oracle against the dense
# solve, 2-norm / Frobenius norm): Q application 6.7e-16 (tiers), 2.7e-16 (many_small);
# clean_bins' S 5.3e-16.  The bounds below are 16 x the largest.
QA_DENSE_BOUND = 16 * 6.7e-16
LMOP_DENSE_BOUND = 16 * 5.3e-16


@pytest.mark.parametrize("name", list(QA))
def test_oracle_interp_is_the_dense_solve(name):
    """row c of interp is A_cc^-1 (b_c + u_c lambda_c), whatever the order of operations: dense
    numpy solves on every support of 1..600 points.  Measured: 6.7e-16 (tiers), 2.7e-16
    (many_small); bound 16 x 6.7e-16"""
    c = QA[name]()
    errs = _qa_dense_errors(c)
    assert len(errs) == ((c.sizes > 0) & (c.sizes <= DENSE_MAX)).sum() >= 20
    print(f"{name}: largest relative error against the dense solve {errs.max():.3e}")
    assert errs.max() <= QA_DENSE_BOUND


def test_oracle_interp_lmop_is_the_dense_sum():
    """clean_bins (qq_chunks has the same operands): S = sum_c u_c P_c A_cc^-1 P_c' on the blocks
    of every support of up to 600 points (the 11 sizes around the QQ^t edges and the chain).
    Measured: 5.3e-16; bound 16 x that"""
    c = wc.lmop_clean_bins()
    errs, n = _lmop_dense_errors(c)
    assert n == (c.sizes <= DENSE_MAX).sum() >= 80
    print(f"clean_bins: largest relative error against the dense sum {errs.max():.3e}")
    assert errs.max() <= LMOP_DENSE_BOUND
