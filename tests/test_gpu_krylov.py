"""Flexible GMRES on the device-resident hierarchy (amgd_krylov_device, amgd_crs_krylov, the
kernel hooks): the ordered path bit for bit against the host restatement tests/refkrylov.py,
the fused path by its residual and its determinism, the orthogonalisation kernels on their
own, and the interface's error returns."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLD
import omp_amg_amd as oa
from omp_amg_amd import abi
import refkrylov
import refsolve
from test_gpu_solve import CRS_A, CRS_I, CRS_J, _coo, same_bits, setup_of

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAXIT = 30
SMALL = ["amgdmp", "aniso_12", "sem_e2_N7", "p27_8", "p7_12"]
RUNS = [(c, r) for c in SMALL for r in (30, 5)] + [("p7_24", 30)]
INFO = ("its", "restarts", "cycles", "converged", "bnorm", "r0", "resid")


@pytest.fixture(autouse=True)
def _defaults():
    oa.init()
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)
    yield
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)


_PROB, _REF = {}, {}


def problem(case):
    """(DeviceSetup, exported hierarchy, b = A x*): x* standard normal, mean removed on a null space"""
    if case not in _PROB:
        ds, h, _, _ = setup_of(case)
        xs = np.random.default_rng(5).standard_normal(int(h.levels[0].n))
        if h.nullspace:
            xs = xs - xs.mean()
        _PROB[case] = (ds, h, refsolve.csr_matvec(h.levels[0].A, xs))
    return _PROB[case]


def ref(case, restart, maxit=MAXIT, guess=False):
    """the restatement's run, computed once and shared"""
    key = (case, restart, maxit, guess)
    if key not in _REF:
        ds, h, b = problem(case)
        x0 = refsolve.vcycle(h, b, remove_mean=bool(h.nullspace)) if guess else None
        _REF[key] = refkrylov.fgmres(h, b, rtol=RTOL, restart=restart, maxit=maxit, x0=x0)
    return _REF[key]


def assert_same_run(got, want, what):
    x, info, hist = got
    assert info["rc"] == want["rc"], (what, info, want["its"])
    for f in INFO:
        assert same_bits(float(info[f]), float(want[f])), (what, f, info[f], want[f])
    assert same_bits(hist, np.array(want["hist"])), (what, hist, want["hist"])
    assert same_bits(x, want["x"]), (what, np.abs(x - want["x"]).max())


# ------------------------------------------------------------------ the ordered path
@pytest.mark.parametrize("case,restart", RUNS)
def test_ordered_path_matches_restatement(case, restart):
    """x, the counts, the norms and every residual estimate bit for bit; db unchanged; a second
    call and the composed cycle give the same bits; with an initial guess; stopped by maxit"""
    ds, h, b = problem(case)
    want = ref(case, restart)
    if case != "p7_24":
        assert want["rc"] == 0 and want["its"] <= 20
    oa.route_stats()
    got = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=True)
    r = oa.route_stats()
    assert_same_run(got, want, "first")
    assert same_bits(ds.b_after, b)
    assert r["kry_odot"] > 0 and r["kry_mdot"] == 0 and r["kry_it"] == want["its"]
    assert_same_run(ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=True), want, "second")
    oa.vc_fused(0)
    assert_same_run(ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=True), want, "composed")
    oa.vc_fused(-1)
    x0 = refsolve.vcycle(h, b, remove_mean=bool(h.nullspace))
    got = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, ordered=True, x0=x0)
    assert_same_run(got, ref(case, restart, guess=True), "guess")
    got = ds.krylov(b, rtol=RTOL, restart=restart, maxit=4, ordered=True)
    want4 = ref(case, restart, maxit=4)
    assert want4["rc"] == 1 and got[1]["rc"] == 1 and got[1]["its"] == 4
    assert_same_run(got, want4, "maxit 4")


# ------------------------------------------------------------------ the fused path
@pytest.mark.parametrize("case,restart", RUNS)
def test_fused_path_converges_and_repeats(case, restart):
    """rc 0 within one iteration of the ordered path's count, the host-recomputed residual at
    most rtol (1 + 1e-3) ||b||, two runs the same bits, only multi-dot launches"""
    ds, h, b = problem(case)
    want = ref(case, restart)
    oa.route_stats()
    x, info, hist = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT)
    r = oa.route_stats()
    assert info["rc"] == 0 and info["converged"] == 1, info
    assert abs(info["its"] - want["its"]) <= 1, (info["its"], want["its"])
    assert same_bits(ds.b_after, b)
    res = np.linalg.norm(b - refsolve.csr_matvec(h.levels[0].A, x)) / np.linalg.norm(b)
    print(case, restart, "its", info["its"], "relative residual", res)
    assert res <= RTOL * (1 + 1e-3), res
    assert r["kry_mdot"] > 0 and r["kry_odot"] == 0 and r["kry_it"] == info["its"]
    x2, info2, hist2 = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT)
    assert same_bits(x2, x) and same_bits(hist2, hist) and info2 == info


# ------------------------------------------------------------------ the kernels on their own
def exact_dots(V, w):
    """per column: (the correctly rounded sum of the exact products, sum |v_i w_i|); a product is
    split without error into its rounded value and the rounding's remainder (Veltkamp / Dekker)"""
    def split(a):
        t = 134217729.0 * a
        hi = t - (t - a)
        return hi, a - hi
    p = V * w[:, None]
    vh, vl = split(V)
    wh, wl = split(w[:, None])
    e = ((vh * wh - p) + vh * wl + vl * wh) + vl * wl
    sums = np.array([math.fsum(np.concatenate([p[:, t], e[:, t]])) for t in range(V.shape[1])])
    return sums, np.abs(p).sum(axis=0)


def same_bits_or_nan(x, y):
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and same_bits(np.where(nx, 0.0, x), np.where(ny, 0.0, y))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_kernel_hooks(n):
    """1, 2, tile - 1, tile, tile + 1 and 65 basis vectors, ld = n and n + 1 with NaN in the
    padding.  The multi-dot: each sum within n u / (1 - n u) sum|v_i w_i| of the exact sum (the
    bound of any summation order, u = 2^-53), the same over two calls.  The update: bit for bit
    the numpy expression, with a -0.0 coefficient and an infinity under a zero coefficient"""
    tile = oa.kry_tile()
    rng = np.random.default_rng(n)
    V, w = rng.standard_normal((n, 65)), rng.standard_normal(n)
    sums, mags = exact_dots(V, w)
    u = 2.0 ** -53
    bound = n * u / (1 - n * u) * mags
    for nb in (1, 2, tile - 1, tile, tile + 1, 65):
        d = rng.standard_normal(nb)
        Vi = V[:, :nb].copy()
        Vi[n // 2, nb - 1] = np.inf
        d[nb - 1] = 0.0
        if nb > 1:
            d[0] = -0.0
        with np.errstate(invalid="ignore"):
            want = w.copy()
            for t in range(nb):
                want = want - d[t] * Vi[:, t]
        assert np.isnan(want[n // 2])
        for ld in (n, n + 1):
            got = oa.test_kry_mdot(V[:, :nb], w, ld)
            assert np.all(np.abs(got - sums[:nb]) <= bound[:nb]), (nb, ld, np.abs(got - sums[:nb]) / mags[:nb])
            assert same_bits(oa.test_kry_mdot(V[:, :nb], w, ld), got), (nb, ld)
            assert same_bits_or_nan(oa.test_kry_update(Vi, w, d, ld), want), (nb, ld)


def test_update_kernel_norm():
    """the partials of ||w||^2 the last update leaves: within the same bound of the exact sum of
    the new w's squares, and its root within one unit in the last place of the host's (the
    solver takes the device's root on both sides, so it asks no more)"""
    n = 4097
    rng = np.random.default_rng(3)
    V, w, d = rng.standard_normal((n, 3)), rng.standard_normal(n), rng.standard_normal(3)
    for ld in (n, n + 1):
        got, nrm = oa.test_kry_update(V, w, d, ld, norm=True)
        s, mag = exact_dots(got[:, None], got)
        u = 2.0 ** -53
        assert abs(nrm[0] - s[0]) <= n * u / (1 - n * u) * mag[0]
        assert abs(nrm[1] - math.sqrt(nrm[0])) <= 2.0 ** -52 * nrm[1]


# ------------------------------------------------------------------ the interface
def raw_call(L, h, dx, db, o, info):
    return L.amgd_krylov_device(h, dx, db, C.byref(o) if o is not None else None,
                                C.byref(info) if info is not None else None, None, 0)


def test_bad_arguments_touch_nothing():
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    ds, h, b = problem("p27_8")
    n = len(b)
    ds.vectors(n)
    nan = np.full(n, np.nan)
    L.amgd_dev_upload(ds.db, b.ctypes.data, b.nbytes)
    L.amgd_dev_upload(ds.dx, nan.ctypes.data, nan.nbytes)
    good, info = abi.KrylovOpts(RTOL, 0.0, 30, 20, 1), abi.KrylovInfo()
    before = L.amgd_test_pool_inuse()
    calls = [(None, ds.dx, ds.db, good, info), (ds.h, None, ds.db, good, info), (ds.h, ds.dx, None, good, info),
             (ds.h, ds.dx, ds.db, None, info), (ds.h, ds.dx, ds.db, good, None)]
    for bad in (abi.KrylovOpts(RTOL, 0.0, 65, 20, 1), abi.KrylovOpts(-1e-3, 0.0, 30, 20, 1),
                abi.KrylovOpts(float("nan"), 0.0, 30, 20, 1), abi.KrylovOpts(RTOL, -1.0, 30, 20, 1),
                abi.KrylovOpts(RTOL, float("nan"), 30, 20, 1)):
        calls.append((ds.h, ds.dx, ds.db, bad, info))
    for k, a in enumerate(calls):
        assert raw_call(L, *a) == -1, k
    L.amgd_dev_sync()
    x = np.zeros(n)
    L.amgd_dev_download(x.ctypes.data, ds.dx, x.nbytes)
    assert np.all(np.isnan(x))
    assert L.amgd_test_pool_inuse() == before


def test_zero_right_hand_side():
    ds, h, b = problem("p27_8")
    for ordered in (True, False):
        x, info, hist = ds.krylov(np.zeros(len(b)), rtol=RTOL, ordered=ordered)
        assert info["rc"] == 0 and info["its"] == 0 and info["converged"] == 1 and len(hist) == 0
        assert same_bits(x, np.zeros(len(b)))


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
        assert L.amgd_comm_partitioned() == 1
        ds = oa.DeviceSetup(Ai, Aj, Av)
        ds.run()
        n = int(np.max(Ai)) + 1
        ds.vectors(n)
        before = L.amgd_test_pool_inuse()
        x, info, _ = ds.krylov(np.ones(n), check=False)
        assert info["rc"] == -3 and np.all(np.isnan(x))
        assert L.amgd_test_pool_inuse() == before
    finally:
        if ds is not None:
            ds.close()
        shard.free()


def test_out_of_hbm_recovers_and_close_frees_the_workspace():
    """a cap below the workspace's need: -2 with the reason, the pool back where it was, dx not
    written, the next call bit-right; the workspace is kept between calls, reused by a smaller
    basis, and gone after close()"""
    L = oa.lib()
    L.amgd_test_hbm_cap.argtypes = [C.c_uint64]
    L.amgd_test_pool_inuse.restype = C.c_uint64
    _, h, b = problem("p7_12")
    n = len(b)
    left = []
    for with_krylov in (False, True):
        ds = oa.DeviceSetup(*_coo("p7_12"))
        try:
            ds.run()
            ds.solve(b)                                   # the plan exists from here on
            if with_krylov:
                before = L.amgd_test_pool_inuse()
                L.amgd_test_hbm_cap(before + 16384)       # V alone is 31 vectors of n doubles
                x, info, _ = ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT, ordered=True, check=False)
                L.amgd_test_hbm_cap(0)
                assert info["rc"] == -2 and b"out of HBM" in L.amgd_error()
                assert np.all(np.isnan(x))
                assert L.amgd_test_pool_inuse() == before
                assert same_bits(ds.solve(b), refsolve.vcycle(h, b))
                assert_same_run(ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT, ordered=True), ref("p7_12", 30), "after")
                kept = L.amgd_test_pool_inuse()
                assert kept - before >= 64 * n * 8
                assert_same_run(ds.krylov(b, rtol=RTOL, restart=5, maxit=MAXIT, ordered=True), ref("p7_12", 5), "m 5")
                assert L.amgd_test_pool_inuse() == kept
        finally:
            L.amgd_test_hbm_cap(0)
            ds.close()
        left.append(L.amgd_test_pool_inuse())
    assert left[1] == left[0], left


# ------------------------------------------------------------------ amgd_crs_krylov
def check_crs(L, hd, ids, b, x0):
    try:
        h = abi.crs_export(L, hd)
        x, info = abi.crs_krylov(L, hd, b, x0=x0, rtol=RTOL, restart=30, maxit=MAXIT, ordered=True)
        assert same_bits(abi.crs_krylov.b_after, b)
    finally:
        L.crs_free(hd)
    want = refkrylov.crs_krylov(h, ids, b, x0=x0, rtol=RTOL, restart=30, maxit=MAXIT)
    assert info["rc"] == want["rc"] == 0
    for f in INFO:
        assert same_bits(float(info[f]), float(want[f])), (f, info[f], want[f])
    assert same_bits(x, want["x"])
    return x


def test_crs_krylov_crs_test_matrix():
    """crs_test.c's 4 x 4 singular Laplacian, null_space = 1, b = id - mean"""
    L = oa.lib()
    ids = np.array([1, 2, 3, 4])
    hd = abi.crs_setup(L, 4, ids, CRS_I, CRS_J, CRS_A, null_space=1)
    assert hd is not None
    check_crs(L, hd, ids, ids - 2.5, None)


def test_crs_krylov_amgdmp_scrambled():
    """amgdmp with scrambled ids, two id-0 dofs and one dof present twice"""
    z = np.load(os.path.join(GOLD, "amgdmp.npz"))
    Ai, Aj, Av = z["in_Ai"].astype(np.int64), z["in_Aj"].astype(np.int64), z["in_Av"]
    n = int(Ai.max()) + 1
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    ids = np.concatenate([perm + 1, [0, 0, perm[5] + 1]])
    xs = rng.standard_normal(n)
    xs -= xs.mean()
    A = abi.Csr(n, n, *_csr_of(inv[Ai], inv[Aj], Av, n))
    bl = refsolve.csr_matvec(A, xs)                     # consistent: in the range of the local matrix
    b = np.concatenate([bl, [3.0, -2.0, 0.0]])
    b[n + 2], b[5] = 0.25 * bl[5], 0.75 * bl[5]          # dof 5's b in two parts
    L = oa.lib()
    hd = abi.crs_setup(L, n + 3, ids, inv[Ai], inv[Aj], Av, null_space=1)
    assert hd is not None
    x = check_crs(L, hd, ids, b, np.full(n + 3, 42.0))
    assert x[n] == 42.0 and x[n + 1] == 42.0 and x[n + 2] == x[5]


def _csr_of(I, J, V, n):
    o = np.lexsort((J, I))
    ro = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))]).astype(np.int64)
    return ro, J[o].astype(np.int64), V[o]


# ------------------------------------------------------------------ statistics
def test_krylov_stats_count_calls_and_iterations():
    ds, h, b = problem("p27_8")
    s0 = oa.krylov_stats()
    _, info, _ = ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT)
    _, info2, _ = ds.krylov(b, rtol=RTOL, restart=5, maxit=MAXIT, ordered=True)
    s1 = oa.krylov_stats()
    assert s1["calls"] == s0["calls"] + 2
    assert s1["its"] == s0["its"] + info["its"] + info2["its"]
    assert s1["ms"] > s0["ms"] >= 0 and s1["ms"] > 0


def test_many_floor_calls_queue_no_timing_events():
    """300 calls of the floor hook (one cycle and one product on the Krylov calls' timer, the cycle
    on the cycles' timer too): the event pairs waiting to be read stay bounded, a stats read
    brings them back to where they stood, and the time has grown"""
    L = oa.lib()
    L.amgd_test_timer_pending.restype = C.c_uint64
    L.amgd_test_kry_floor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.amgd_test_kry_floor.restype = C.c_int
    ds, h, b = problem("p7_12")
    ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT)       # the workspace
    oa.solve_stats()                  # read what is pending
    ms0 = oa.krylov_stats()["ms"]
    base = L.amgd_test_timer_pending()
    seen = 0
    for k in range(300):
        assert L.amgd_test_kry_floor(ds.h, ds.dx, ds.db) == 0
        seen = max(seen, L.amgd_test_timer_pending())
    print("pending: base", base, "max", seen)
    assert seen - base <= 256, (base, seen)
    oa.solve_stats()
    st = oa.krylov_stats()
    assert L.amgd_test_timer_pending() == base
    assert st["ms"] > ms0
