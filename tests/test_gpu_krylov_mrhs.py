"""Flexible GMRES on several right-hand sides (amgd_krylov_device_n, amgd_crs_krylov_n, the
kernel hooks): every column bit for bit the single solver's run on the same device pointers,
whatever the slot count and the group sizes; the K-column level-0 product against the host
restatement of amgd_spmv; the multi-column orthogonalisation kernels against the single ones;
the interface's error returns.

The reference of a column is amgd_krylov_device on that column of the same device blocks
(DeviceSetup.krylov_at) -- the contract's own words.  DeviceSetup.krylov, which uploads the
column to 16-byte aligned vectors of its own, is compared as well wherever the alignment cannot
matter: on the ordered path (left-to-right sums) for every column, on the fused path for the
columns that start 16-byte aligned in the block (with ld = n0 + 3 odd, the even ones; the fused
||b|| takes the paired or the unpaired multi-dot by the pointer it is given)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import omp_amg_amd as oa
from omp_amg_amd import abi
import krylov_mrhs_inputs as kin
import refsolve
from test_gpu_krylov import INFO, _csr_of, same_bits_or_nan
from test_gpu_solve import _coo, same_bits, setup_of

pytestmark = pytest.mark.gpu

RTOL, MAXIT, NC = kin.RTOL, kin.MAXIT, kin.NCOLS


@pytest.fixture(autouse=True)
def _defaults():
    oa.init()
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)
    oa.vc_mrhs_k((2, 4, 8))        # every group size and 8 slots, whatever the shipped defaults allow
    oa.kry_slots(8)
    oa.kry_family(-1)
    yield
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail, oa.vc_mrhs_k, oa.kry_slots, oa.kry_family):
        f(-1)


def problem(case):
    ds, h, _, _ = setup_of(case)
    XS, B, X0 = kin.inputs(case, h)
    return ds, h, B, X0


def pad_of(n0):
    return n0 + 3


_SINGLE = {}


def singles(case, restart, ordered, guess, cols=None):
    """amgd_krylov_device on every column of the device blocks (the same pointers the multi-RHS
    call is given), computed once per combination and shared"""
    key = (case, restart, ordered, guess, None if cols is None else tuple(cols))
    if key not in _SINGLE:
        ds, h, B, X0 = problem(case)
        if cols is not None:
            B, X0 = B[:, cols], X0[:, cols]
        n0, ld = B.shape[0], pad_of(B.shape[0])
        ds.krylov_n(B, rtol=RTOL, restart=restart, maxit=1, ordered=ordered, ld=ld)      # B's block in place
        ds.krylov_n_blocks(X0 if guess else np.full_like(B, np.nan), ld)
        _SINGLE[key] = [ds.krylov_at(j, ld, n0, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=ordered, guess=guess)
                        for j in range(B.shape[1])]
    return _SINGLE[key]


def assert_columns(got, want, what):
    X, infos, hists = got
    assert len(infos) == len(want)
    for j, (x, info, hist) in enumerate(want):
        assert infos[j]["rc"] == info["rc"], (what, j, infos[j], info)
        for f in INFO:
            assert same_bits(float(infos[j][f]), float(info[f])), (what, j, f, infos[j][f], info[f])
        assert same_bits(hists[j], hist), (what, j, hists[j], hist)
        assert same_bits_or_nan(X[:, j], x), (what, j)


def run_n(ds, B, X0, restart, ordered, guess):
    n0 = B.shape[0]
    got = ds.krylov_n(B, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=ordered, X0=X0 if guess else None,
                      ld=pad_of(n0))
    assert same_bits(ds.B_after, B)
    assert ds.X_pad.shape == (3, B.shape[1]) and np.all(np.isnan(ds.X_pad))
    return got


# ------------------------------------------------------------------ columns equal the single solver
@pytest.mark.parametrize("guess", [True, False], ids=["guess", "zero"])
@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "fused"])
@pytest.mark.parametrize("restart", [30, 5])
@pytest.mark.parametrize("case", kin.CASES)
def test_columns_equal_the_single_solver(case, restart, ordered, guess):
    """x, every info field, rc and the history of each of the 8 columns; B unchanged, the padding
    still NaN; the same bits with 3 slots and with 1, and with the group sizes 8,4,2 / 2 / none.
    With 3 slots, the guesses and restart 5 the columns hand their slots on and stand at
    different inner indices, and the products run through the K-column kernel."""
    ds, h, B, X0 = problem(case)
    want = singles(case, restart, ordered, guess)
    assert all(w[1]["rc"] == 0 for w in want)
    assert_columns(run_n(ds, B, X0, restart, ordered, guess), want, "8 slots")
    for slots in (3, 1):
        oa.kry_slots(slots)
        oa.route_stats()
        got = run_n(ds, B, X0, restart, ordered, guess)
        r = oa.route_stats()
        assert_columns(got, want, f"{slots} slots")
        assert r["kry_it"] == sum(i["its"] for i in got[1]), r
        assert (r["kry_mdot"] == 0) if ordered else (r["kry_odot"] == 0), r
        if slots == 3 and guess and restart == 5:
            assert r["kry_n_mixed"] > 0 and r["kry_n_prod"] > 0 and r["kry_n_step"] >= r["kry_n_mixed"], r
        if slots == 1:
            assert r["kry_n_prod"] == 0 and r["kry_n_mixed"] == 0, r
    oa.kry_slots(8)
    for sizes in ((2,), ()):
        oa.vc_mrhs_k(sizes)
        oa.route_stats()
        assert_columns(run_n(ds, B, X0, restart, ordered, guess), want, f"groups {sizes}")
        r = oa.route_stats()
        assert (r["kry_n_prod"] > 0) == bool(sizes) and (r["vc_mr_thr"] + r["vc_mr_wave"] > 0) == bool(sizes), r
    oa.vc_mrhs_k((2, 4, 8))
    if restart == 5:
        # DeviceSetup.krylov on the column alone, where the alignment cannot matter (module docstring)
        n0 = B.shape[0]
        for j in range(NC):
            if ordered or (j * pad_of(n0)) % 2 == 0:
                x, info, hist = ds.krylov(B[:, j], rtol=RTOL, restart=restart, maxit=MAXIT, ordered=ordered,
                                          x0=X0[:, j] if guess else None)
                assert_columns((x[:, None], [info], [hist]), [want[j]], f"krylov() column {j}")
        if ordered and guess:                      # once per fixture: the host restatement itself
            for j, res in enumerate(kin.reference(case, h, restart, True)):
                x, info, hist = want[j]
                assert info["rc"] == res["rc"] and info["its"] == res["its"], (j, info, res["its"])
                assert same_bits(hist, np.array(res["hist"])) and same_bits(x, res["x"]), j


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "fused"])
def test_every_number_of_columns(ordered):
    """nrhs 1, 2, 3, 5, 8 and 11 (columns repeated), the guesses, restart 5"""
    case = "p27_8"
    ds, h, B, X0 = problem(case)
    for nrhs in (1, 2, 3, 5, 8, 11):
        cols = [j % NC for j in range(nrhs)]
        want = singles(case, 5, ordered, True, cols=cols)
        oa.route_stats()
        assert_columns(run_n(ds, B[:, cols], X0[:, cols], 5, ordered, True), want, f"nrhs {nrhs}")
        r = oa.route_stats()
        # two columns: column 1 (its guess is the solution) ends at once and leaves column 0 alone
        assert r["kry_n_prod"] == 0 if nrhs == 1 else r["kry_n_prod"] > 0 or nrhs == 2, (nrhs, r)


# ------------------------------------------------------------------ the product kernel on its own
def rand_csr(rng, n, mean, long_row=0, empty=True, base=0):
    """n x n, row lengths base + Poisson(mean) (some rows empty), row n // 2 of long_row entries;
    columns ascending, drawn with replacement (a product does not care)"""
    lens = base + rng.poisson(mean, n)
    if empty:
        lens[rng.integers(0, n, max(1, n // 8))] = 0
    if long_row:
        lens[n // 2] = long_row
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.integers(0, n, k)) for k in lens] + [np.zeros(0, dtype=np.int64)])
    return abi.Csr(n, n, ro, col.astype(np.int64), rng.standard_normal(int(ro[-1])))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_product_kernel(n):
    """Z_j = A X_j and Z_j = 1*B_j + (-1)*(A X_j) bit for bit refsolve.apply_M per column: K = 2,
    4, 8, both kernel families on a short-row matrix (mean 6, empty rows, one row of 300), a
    long-row matrix (rows of 32 + Poisson(8)) and a matrix with a row of 4 097 entries (column by column through
    the single-vector product); the columns at unrelated pointers, some aligned to 8 bytes only;
    a -0.0 and an infinity among the operands"""
    rng = np.random.default_rng(100 + n)
    mats = {"short": rand_csr(rng, n, 6.0, long_row=300), "long": rand_csr(rng, n, 8.0, empty=False, base=32),
            "outlier": rand_csr(rng, n, 6.0, long_row=4097)}
    assert mats["long"].nnz >= 32 * n
    X, Y = rng.standard_normal((n, 8)), rng.standard_normal((n, 8))
    X[0, 0] = -0.0
    X[n // 3, 1] = np.inf
    for name, A in mats.items():
        want = {}
        for j in range(8):
            with np.errstate(invalid="ignore", over="ignore"):
                want[j] = (refsolve.apply_M(A, X[:, j]), refsolve.apply_M(A, X[:, j], 1.0, Y[:, j], -1.0))
        for K in (2, 4, 8):
            for fam in ("short", "long"):
                for form in (0, 1):
                    oa.route_stats()
                    Z = oa.test_kry_spmv_n(A, X[:, :K], *((1.0, Y[:, :K], -1.0) if form else (0.0, None, 1.0)),
                                           family=fam, shift=0b10110110)
                    r = oa.route_stats()
                    for j in range(K):
                        assert same_bits_or_nan(Z[:, j], want[j][form]), (name, K, fam, form, j)
                    if name == "outlier":
                        assert r["kry_n_comp"] == K and r["kry_n_prod"] == 0, r
                    else:
                        assert r["kry_n_prod"] == 1 and r["kry_n_comp"] == 0 and r["kry_n_single"] == 0, r


# ------------------------------------------------------------------ the multi-column Gram-Schmidt kernels
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_multi_column_orthogonalisation_kernels(n):
    """3 columns with 1, tile - 1, tile + 1 or 65 basis vectors each, ld = n and n + 1: every
    column bit for bit the single hooks on that column with the same ld (the norm's partials
    too)"""
    tile = oa.kry_tile()
    rng = np.random.default_rng(200 + n)
    for nbs in ((1, tile - 1, 65), (tile + 1, 65, 1), (65, 1, tile - 1), (tile - 1, tile + 1, tile + 1)):
        Vs = [rng.standard_normal((n, nb)) for nb in nbs]
        ws = [rng.standard_normal(n) for _ in nbs]
        ds_ = [rng.standard_normal(nb) for nb in nbs]
        for ld in (n, n + 1):
            dots = oa.test_kry_mdot_n(Vs, ws, ld)
            upd = oa.test_kry_update_n(Vs, ws, ds_, ld)
            updn = oa.test_kry_update_n(Vs, ws, ds_, ld, norm=True)
            for q in range(3):
                assert same_bits(dots[q], oa.test_kry_mdot(Vs[q], ws[q], ld)), (nbs, ld, q)
                assert same_bits(upd[q], oa.test_kry_update(Vs[q], ws[q], ds_[q], ld)), (nbs, ld, q)
                w1, nrm1 = oa.test_kry_update(Vs[q], ws[q], ds_[q], ld, norm=True)
                assert same_bits(updn[q][0], w1) and same_bits(updn[q][1], nrm1), (nbs, ld, q)


# ------------------------------------------------------------------ the interface
def test_bad_arguments_touch_nothing():
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    ds, h, B, X0 = problem("p27_8")
    n0 = B.shape[0]
    run_n(ds, B, X0, 5, False, False)                      # the blocks and the workspace exist
    ds.krylov_n_blocks(np.full_like(B, np.nan), pad_of(n0))
    good = abi.KrylovOpts(RTOL, 0.0, 30, 20, 0)
    infos, rcs = (abi.KrylovInfo * NC)(), (C.c_int * NC)(*([7] * NC))
    before = L.amgd_test_pool_inuse()
    ld = pad_of(n0)

    def call(h_=ds.h, dx=ds.dxn, db=ds.dbn, nrhs=NC, ld_=ld, o=good, info=infos):
        return L.amgd_krylov_device_n(h_, dx, db, nrhs, ld_, C.byref(o) if o is not None else None, info, rcs,
                                      None, 0)
    bad = [call(h_=None), call(dx=None), call(db=None), call(o=None), call(info=None), call(nrhs=0),
           call(nrhs=-1), call(ld_=n0 - 1)]
    for o in (abi.KrylovOpts(RTOL, 0.0, 65, 20, 0), abi.KrylovOpts(-1e-3, 0.0, 30, 20, 0),
              abi.KrylovOpts(float("nan"), 0.0, 30, 20, 0), abi.KrylovOpts(RTOL, -1.0, 30, 20, 0),
              abi.KrylovOpts(RTOL, float("nan"), 30, 20, 0)):
        bad.append(call(o=o))
    assert bad == [-1] * len(bad), bad
    L.amgd_dev_sync()
    x = np.zeros((NC, ld))
    L.amgd_dev_download(x.ctypes.data, ds.dxn, x.nbytes)
    assert np.all(np.isnan(x)) and list(rcs) == [7] * NC
    assert L.amgd_test_pool_inuse() == before


def test_rejects_partitioned_hierarchy():
    """a hierarchy of the partitioned driver (one-rank RCCL communicator): -3, nothing allocated"""
    from omp_amg_amd import shard
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    Ai, Aj, Av = _coo("p7_12")
    uid = C.create_string_buffer(128)
    assert L.amgd_comm_rccl_uid(uid) == 0
    assert L.amgd_comm_init_rccl(0, 1, uid.raw) == 0
    ds = None
    try:
        L.amgd_comm_set_partitioned(1)
        ds = oa.DeviceSetup(Ai, Aj, Av)
        ds.run()
        n = int(np.max(Ai)) + 1
        ds.krylov_n(np.ones((n, 2)), check=False)          # the blocks exist from here on
        before = L.amgd_test_pool_inuse()
        X, infos, _ = ds.krylov_n(np.ones((n, 2)), check=False)
        assert ds.rc_n == -3 and np.all(np.isnan(X))
        assert L.amgd_test_pool_inuse() == before
    finally:
        if ds is not None:
            ds.close()
        shard.free()


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "fused"])
def test_zero_and_non_finite_columns(ordered):
    """a zero column among the others ends with its 0 and x 0; a column with an infinity gets
    rcs -4 and stays NaN, the others are bit-right and the call returns -4"""
    case = "p27_8"
    ds, h, B, X0 = problem(case)
    want = singles(case, 30, ordered, False)
    Bz = B.copy()
    Bz[:, 2] = 0.0
    X, infos, hists = run_n(ds, Bz, X0, 30, ordered, False)
    assert ds.rc_n == 0
    assert infos[2]["rc"] == 0 and infos[2]["its"] == 0 and infos[2]["converged"] == 1 and len(hists[2]) == 0
    assert same_bits(X[:, 2], np.zeros(len(B)))
    keep = [j for j in range(NC) if j != 2]
    assert_columns((X[:, keep], [infos[j] for j in keep], [hists[j] for j in keep]), [want[j] for j in keep], "zero")
    Bi = B.copy()
    Bi[5, 3] = np.inf
    X, infos, hists = ds.krylov_n(Bi, rtol=RTOL, restart=30, maxit=MAXIT, ordered=ordered, ld=pad_of(len(B)))
    assert ds.rc_n == -4 and infos[3]["rc"] == -4 and np.all(np.isnan(X[:, 3]))
    keep = [j for j in range(NC) if j != 3]
    assert_columns((X[:, keep], [infos[j] for j in keep], [hists[j] for j in keep]), [want[j] for j in keep], "inf")


def test_out_of_hbm_recovers_and_close_frees_the_workspace():
    """a cap below the slots' workspace: -2, the pool back where it was, nothing written, the next
    call bit-right; close() frees the workspace"""
    L = oa.lib()
    L.amgd_test_hbm_cap.argtypes = [C.c_uint64]
    L.amgd_test_pool_inuse.restype = C.c_uint64
    case = "p7_12"
    _, h, B, X0 = problem(case)
    want = singles(case, 30, False, False)
    n0 = len(B)
    left = []
    for with_krylov in (False, True):
        ds = oa.DeviceSetup(*_coo(case))
        try:
            ds.run()
            ds.solve(B[:, 0])                             # the plan, its tail, its interleaved vectors
            ds.solve_n(B, ld=pad_of(n0))                  # and the device blocks exist from here on
            if with_krylov:
                before = L.amgd_test_pool_inuse()
                L.amgd_test_hbm_cap(before + 16384)       # 8 slots of 64 vectors
                X, infos, _ = ds.krylov_n(B, rtol=RTOL, restart=30, maxit=MAXIT, ld=pad_of(n0), check=False)
                L.amgd_test_hbm_cap(0)
                assert ds.rc_n == -2 and b"out of HBM" in L.amgd_error()
                assert np.all(np.isnan(X)) and L.amgd_test_pool_inuse() == before
                assert_columns(run_n(ds, B, X0, 30, False, False), want, "after")
                assert L.amgd_test_pool_inuse() - before >= 8 * 64 * n0 * 8
        finally:
            L.amgd_test_hbm_cap(0)
            ds.close()
        left.append(L.amgd_test_pool_inuse())
    assert left[1] == left[0], left


def test_crs_krylov_n_amgdmp_scrambled():
    """amgdmp with scrambled ids, two id-0 dofs and one dof present twice (the case of
    test_gpu_krylov.py): every column what amgd_crs_krylov gives on it"""
    z = np.load(os.path.join(GOLD, "amgdmp.npz"))
    Ai, Aj, Av = z["in_Ai"].astype(np.int64), z["in_Aj"].astype(np.int64), z["in_Av"]
    n = int(Ai.max()) + 1
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    ids = np.concatenate([perm + 1, [0, 0, perm[5] + 1]])
    A = abi.Csr(n, n, *_csr_of(inv[Ai], inv[Aj], Av, n))
    cols, B = 3, np.zeros((n + 3, 3))
    for j in range(cols):
        xs = rng.standard_normal(n)
        bl = refsolve.csr_matvec(A, xs - xs.mean())
        B[:, j] = np.concatenate([bl, [3.0, -2.0, 0.0]])
        B[n + 2, j], B[5, j] = 0.25 * bl[5], 0.75 * bl[5]
    X0 = np.full((n + 3, cols), 42.0)
    L = oa.lib()
    hd = abi.crs_setup(L, n + 3, ids, inv[Ai], inv[Aj], Av, null_space=1)
    assert hd is not None
    try:
        for guess in (False, True):
            rc, X, infos = abi.crs_krylov_n(L, hd, B, X0=X0, ld=n + 5, rtol=RTOL, restart=5, maxit=MAXIT,
                                            ordered=True, guess=guess)
            assert rc == 0 and same_bits(abi.crs_krylov_n.b_after, B)
            for j in range(cols):
                x, info = abi.crs_krylov(L, hd, B[:, j], x0=X0[:, j], rtol=RTOL, restart=5, maxit=MAXIT,
                                         ordered=True, guess=guess)
                assert info["rc"] == infos[j]["rc"] == 0
                for f in INFO:
                    assert same_bits(float(info[f]), float(infos[j][f])), (guess, j, f)
                assert same_bits(X[:, j], x), (guess, j)
                assert X[n, j] == 42.0 and X[n + 1, j] == 42.0 and X[n + 2, j] == X[5, j]
    finally:
        L.crs_free(hd)


def test_krylov_n_stats_count_calls_columns_and_steps():
    ds, h, B, X0 = problem("p27_8")
    s0 = oa.krylov_n_stats()
    oa.route_stats()
    _, infos, _ = run_n(ds, B, X0, 5, False, True)
    steps = oa.route_stats()["kry_n_step"]
    run_n(ds, B[:, :3], X0[:, :3], 30, True, False)
    s1 = oa.krylov_n_stats()
    assert s1["calls"] == s0["calls"] + 2 and s1["columns"] == s0["columns"] + NC + 3
    assert s1["steps"] - s0["steps"] == steps + oa.route_stats()["kry_n_step"]
    assert steps >= max(i["its"] for i in infos)
    assert s1["ms"] > s0["ms"] >= 0


def test_many_floor_calls_queue_no_timing_events():
    """300 calls of the 2-column floor hook (a lock-step step's cycles and products on the
    multi-RHS Krylov calls' timer): the event pairs waiting to be read stay bounded, a stats read
    brings them back to where they stood, and the time has grown"""
    L = oa.lib()
    L.amgd_test_timer_pending.restype = C.c_uint64
    L.amgd_test_kry_floor_n.argtypes = [C.c_void_p, C.c_int]
    L.amgd_test_kry_floor_n.restype = C.c_int
    ds, h, B, X0 = problem("p7_12")
    run_n(ds, B[:, :2], X0[:, :2], 30, False, False)       # the slots
    oa.solve_stats()                  # read what is pending
    ms0 = oa.krylov_n_stats()["ms"]
    base = L.amgd_test_timer_pending()
    seen = 0
    for k in range(300):
        assert L.amgd_test_kry_floor_n(ds.h, 2) == 0
        seen = max(seen, L.amgd_test_timer_pending())
    print("pending: base", base, "max", seen)
    assert seen - base <= 256, (base, seen)
    oa.solve_stats()
    st = oa.krylov_n_stats()
    assert L.amgd_test_timer_pending() == base
    assert st["ms"] > ms0
