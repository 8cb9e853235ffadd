"""The interpolation loop's reuse of what a skeleton already knows: transposes by the
skeleton's own transpose map (amgd_untranspose_by_perm / amgd_transpose_by_perm, test ops
21 / 23), W.*(Arhat + Ar) without the sum matrix (amgd_mxmpoint_sum, op 22), and the
driver with each of the two switched off.  Everything is compared bit for bit (values as
uint64, so -0.0 and NaN payloads count).

Shapes 37 x 29 and 300 x 200, each sparse (the per-thread kernels) and dense (the
per-wavefront ones: amgd_rows_strict goes wave-per-row from a mean row of 16 entries,
amgd_mxmpoint_sum from 32 entries per row over its three operands; amgd_mpm, the two-step
reference, takes its wave form on rows of 64 entries and more).  The 130-entry row is in
the 300 x 200 matrices; a duplicate-free row of a 29-column matrix cannot hold 130 entries,
so there the long row is every column that is not kept empty.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import omp_amg_amd as oa
from omp_amg_amd import abi, parity, problems

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29), (300, 200)]
LONG = 130
LONG_ROW, SHORT_ROW = 7, 2


def _csr(mask, vals):
    rn, cn = mask.shape
    ro = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    i, j = np.nonzero(mask)                      # row-major: columns ascending within a row
    return abi.Csr(rn, cn, ro, j.astype(np.int64), np.ascontiguousarray(vals[i, j], dtype=np.float64))


def _same(X, Y):
    return (X.rn, X.cn) == (Y.rn, Y.cn) and np.array_equal(X.row_off, Y.row_off) and \
        np.array_equal(X.col, Y.col) and np.array_equal(X.a.view(np.uint64), Y.a.view(np.uint64))


def _long_cols(cn):
    """columns of the long row: LONG of them from column 10 on, or all but the empty ones"""
    keep = np.ones(cn, dtype=bool)
    keep[[4, cn - 1]] = False                    # the empty columns
    c = np.nonzero(keep)[0]
    return c[c >= 10][:LONG] if cn > LONG + 12 else c


def _tr_matrix(rn, cn, dense, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((rn, cn)) < (0.8 if dense else 0.04)
    mask[LONG_ROW, :] = False
    mask[LONG_ROW, _long_cols(cn)] = True
    mask[[5, rn - 1], :] = False                 # empty rows
    mask[:, [4, cn - 1]] = False                 # empty columns
    vals = rng.standard_normal((rn, cn))
    i, j = np.nonzero(mask)
    vals[i[1], j[1]] = 0.0
    vals[i[3], j[3]] = -0.0
    vals[i[-2], j[-2]] = np.nan
    k = np.nonzero(i == LONG_ROW)[0]
    vals[LONG_ROW, j[k[5]]] = -0.0
    vals[LONG_ROW, j[k[6]]] = np.frombuffer(np.uint64(0x7ff8000000abcdef).tobytes(), dtype=np.float64)[0]
    return _csr(mask, vals)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_untranspose_by_map_returns_the_matrix(shape, dense):
    A = _tr_matrix(*shape, dense, seed=11)
    if shape[1] > LONG + 12:
        assert A.row_off[LONG_ROW + 1] - A.row_off[LONG_ROW] == LONG
    assert _same(oa.test_csr_op(21, A), A)
    # ... which is what the sort gives for the transpose of the transpose
    assert _same(oa.test_csr_op(1, oa.test_csr_op(1, A)), A)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_transpose_by_map_equals_transpose(shape, dense):
    A = _tr_matrix(*shape, dense, seed=12)
    assert _same(oa.test_csr_op(23, A), oa.test_csr_op(1, A))


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_unsorted_row_takes_the_sort(dense):
    """two entries of one row swapped: the row is no longer increasing, the stable transpose
    of the transpose is the sorted matrix and not the input, and op 21 must return it"""
    A = _tr_matrix(37, 29, dense, seed=13)
    r = 9 if A.row_off[10] - A.row_off[9] >= 2 else LONG_ROW
    s = int(A.row_off[r])
    col, a = A.col.copy(), A.a.copy()
    col[[s, s + 1]] = col[[s + 1, s]]
    a[[s, s + 1]] = a[[s + 1, s]]
    U = abi.Csr(A.rn, A.cn, A.row_off, col, a)
    X = oa.test_csr_op(21, U)
    assert _same(X, A)
    assert _same(X, oa.test_csr_op(1, oa.test_csr_op(1, U)))
    assert not _same(X, U)
    # the gather direction holds for any row order
    assert _same(oa.test_csr_op(23, U), oa.test_csr_op(1, U))


def _sum_case(rn, cn, dense, seed, a_empty=False, b2_empty=False):
    """A, B1, B2 with, in the short row and in the long one, a column of each kind: in A and
    B1 only, in A and B2 only, in all three with a non-zero sum, in all three with
    b2 = -b1 (dropped), in A only; elsewhere random, B-only columns included"""
    rng = np.random.default_rng(seed)
    p = 0.5 if dense else 0.03
    mA, m1, m2 = (rng.random((rn, cn)) < p for _ in range(3))
    lc = _long_cols(cn)
    mA[LONG_ROW, :] = False
    mA[LONG_ROW, lc] = True
    for r, c0 in ((SHORT_ROW, 0), (LONG_ROW, int(lc[0]))):
        c = np.arange(c0, c0 + 5)
        mA[r, c] = True
        m1[r, c] = [True, False, True, True, False]
        m2[r, c] = [False, True, True, True, False]
    for m in (mA, m1, m2):
        m[[5, rn - 1], :] = False
    if a_empty:
        mA[:] = False
    if b2_empty:
        m2[:] = False
    vA, v1, v2 = (rng.standard_normal((rn, cn)) for _ in range(3))
    cancel = m1 & m2 & (rng.random((rn, cn)) < 0.3)
    cancel[SHORT_ROW, 3] = True
    cancel[LONG_ROW, int(lc[0]) + 3] = True
    cancel[SHORT_ROW, 2] = False
    cancel[LONG_ROW, int(lc[0]) + 2] = False
    v2[cancel] = -v1[cancel]
    vA[SHORT_ROW, 1] = 0.0                       # zeros of A are kept, as in mxmpoint
    return _csr(mA, vA), _csr(m1, v1), _csr(m2, v2), cancel & mA


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mxmpoint_sum_equals_two_steps(shape, dense):
    A, B1, B2, dropped = _sum_case(*shape, dense, seed=21)
    X = oa.test_csr_op3(22, A, B1, B2)
    ref = oa.test_csr_op(3, A, oa.test_csr_op(2, B1, B2))
    assert _same(X, ref)
    # the fixture did what it says: dropped pairs under A exist and are absent from X
    assert dropped[SHORT_ROW].any() and dropped[LONG_ROW].any()
    dense_x = np.zeros(shape, dtype=bool)
    for i in range(X.rn):
        dense_x[i, X.col[X.row_off[i]:X.row_off[i + 1]]] = True
    assert not (dense_x & dropped).any()
    assert dense_x[SHORT_ROW, :3].all() and not dense_x[SHORT_ROW, 3:5].any()


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("which", ["a_empty", "b2_empty"])
def test_mxmpoint_sum_empty_operand(which, dense):
    A, B1, B2, _ = _sum_case(300, 200, dense, seed=22, **{which: True})
    assert (A.nnz == 0) == (which == "a_empty") and (B2.nnz == 0) == (which == "b2_empty")
    X = oa.test_csr_op3(22, A, B1, B2)
    assert _same(X, oa.test_csr_op(3, A, oa.test_csr_op(2, B1, B2)))
    if which == "a_empty":
        assert X.nnz == 0


# ---------------------------------------------------------------- the driver
def _inputs(case):
    return problems.poisson3d(12) if case == "p7_12" else problems.poisson3d(16)


@pytest.fixture(scope="module", params=["p7_12", "p7_16"])
def four_hierarchies(request):
    Ai, Aj, Av = _inputs(request.param)
    out = {}
    try:
        for tr in (1, 0):
            for fuse in (1, 0):
                oa.skel_tr(tr)
                oa.fuse_arr(fuse)
                oa.route_stats(reset=True)
                h = abi.run_setup(oa.lib(), Ai, Aj, Av)
                out[(tr, fuse)] = (h, oa.route_stats(reset=True))
    finally:
        oa.skel_tr(-1)
        oa.fuse_arr(-1)
    return request.param, out


def test_driver_switches_give_one_hierarchy(four_hierarchies):
    case, hs = four_hierarchies
    base = hs[(1, 1)][0]
    if case == "p7_12":
        z = np.load(os.path.join(GOLD, "p7_12.npz"))
        assert parity.first_diff(parity.from_npz(z), base) == []
    for key in ((0, 1), (1, 0), (0, 0)):
        assert parity.first_diff(base, hs[key][0]) == [], key


def test_driver_takes_the_map_route(four_hierarchies):
    _, hs = four_hierarchies
    assert hs[(1, 1)][1]["skel_tr"] > 0 and hs[(1, 0)][1]["skel_tr"] > 0
    assert hs[(0, 1)][1]["skel_tr"] == 0 and hs[(0, 0)][1]["skel_tr"] == 0


def test_kept_map_is_released():
    oa.init()
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    before = L.amgd_test_pool_inuse()
    ds = oa.DeviceSetup(*problems.poisson3d(12))
    oa.route_stats(reset=True)
    ds.run()
    assert oa.route_stats(reset=True)["skel_tr"] > 0
    ds.close()
    assert L.amgd_test_pool_inuse() == before
