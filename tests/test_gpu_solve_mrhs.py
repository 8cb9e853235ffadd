"""The V-cycle on several right-hand sides (amgd_solve_device_n, amgd_crs_solve_n, the K-column
level hooks) -- column j bit for bit what the single-vector cycle gives on column j.
Yardsticks: tests/refsolve.py per column, and the single-vector DeviceSetup.solve, which
tests/test_gpu_solve.py pins to refsolve."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import omp_amg_amd as oa
from omp_amg_amd import abi, problems
import mrhs_inputs
import refsolve

pytestmark = pytest.mark.gpu

KS = (2, 4, 8)
NRHS = (1, 2, 3, 4, 5, 8, 11)
FAMILIES = ("short", "long")
CRS_A = np.array([2, -1, -1, 0, -1, 2, 0, -1, -1, 0, 2, -1, 0, -1, -1, 2], dtype=np.float64)
CRS_I = np.repeat(np.arange(4), 4)
CRS_J = np.tile(np.arange(4), 4)


def same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.fixture(autouse=True)
def _defaults():
    oa.init()
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)
    oa.vc_rw(0)
    oa.vc_mrhs_k((2, 4, 8))        # every group size, whatever the shipped default allows
    yield
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail, oa.vc_mrhs_k):
        f(-1)
    oa.vc_rw(0)


# ------------------------------------------------------------------ whole hierarchies
def _coo(case):
    if case == "p7_24":
        return problems.poisson3d(24)
    z = np.load(os.path.join(GOLD, case + ".npz"))
    return z["in_Ai"], z["in_Aj"], z["in_Av"]


_SETUPS = {}


def setup_of(case):
    """one setup per case for the module: (DeviceSetup, hierarchy, B, reference block per flag);
    the references are computed once: refsolve per column, p7_24 (no golden file, slow in the
    restatement) the single-vector solve per column"""
    if case not in _SETUPS:
        ds = oa.DeviceSetup(*_coo(case))
        ds.run()
        h = ds.export()
        n0 = int(h.levels[0].n)
        B = mrhs_inputs.block(n0)
        ref = {}
        for f in (False, True):
            if case == "p7_24":
                cols = [ds.solve(B[:, j], remove_mean=f) for j in range(B.shape[1])]
            else:
                cols = [refsolve.vcycle(h, B[:, j], remove_mean=f) for j in range(B.shape[1])]
            ref[f] = np.stack(cols, axis=1)
        _SETUPS[case] = (ds, h, B, ref)
    return _SETUPS[case]


@pytest.mark.parametrize("case", mrhs_inputs.CASES)
def test_solve_n_matches_reference(case):
    """prefixes of an 11-column block (one all-zero column, one of +-0.0 and denormals), with and
    without the mean, ld = n0 and n0 + 3 (NaN in X's padding before and after), B unchanged, a
    second call the same; then with each single group size allowed"""
    ds, h, B, ref = setup_of(case)
    n0 = B.shape[0]
    assert np.all(np.isfinite(ref[False])) and np.all(np.isfinite(ref[True]))
    for sizes in ((2, 4, 8), (2,), (4,), (8,)):
        oa.vc_mrhs_k(sizes)
        for nrhs in NRHS:
            for flag in (False, True):
                for ld in (n0, n0 + 3):
                    X = ds.solve_n(B[:, :nrhs], remove_mean=flag, ld=ld)
                    bad = [j for j in range(nrhs) if not same_bits(X[:, j], ref[flag][:, j])]
                    assert not bad, (case, sizes, nrhs, flag, ld, bad)
                    assert same_bits(ds.B_after, B[:, :nrhs])
                    assert ds.X_pad.shape == (ld - n0, nrhs) and np.all(np.isnan(ds.X_pad))
            X2 = ds.solve_n(B[:, :nrhs])
            assert same_bits(X2, ref[False][:, :nrhs]), (case, sizes, nrhs)


def test_single_solves_around_solve_n():
    """solve, solve_n, solve: the single results are identical, and the single-vector cycle count
    advances by the single calls plus the columns solve_n sent through the single-vector cycle"""
    ds, h, B, ref = setup_of("p7_12")
    b = B[:, 1]
    oa.route_stats()
    c0 = oa.solve_stats()["cycles"]
    n0 = oa.solve_n_stats()
    x1 = ds.solve(b)
    X = ds.solve_n(B[:, :7], remove_mean=True)          # 4 + 2 + 1
    x2 = ds.solve(b)
    r = oa.route_stats()
    n1 = oa.solve_n_stats()
    assert same_bits(x1, ref[False][:, 1]) and same_bits(x2, x1)
    assert same_bits(X, ref[True][:, :7])
    assert r["vc_mr_single"] == 1
    assert oa.solve_stats()["cycles"] - c0 == 2 + r["vc_mr_single"]
    assert n1["calls"] - n0["calls"] == 1 and n1["columns"] - n0["columns"] == 7
    assert n1["ms"] > n0["ms"]
    one = oa.solve_stats()["bytes"]
    assert one < n1["bytes"] < 7 * one                   # the matrices once per group


def test_solve_n_routes():
    ds, h, B, ref = setup_of("p7_24")
    oa.route_stats()
    ds.solve_n(B[:, :4])
    r = oa.route_stats()
    assert r["vc_mr_thr"] > 0 and r["vc_mr_wave"] > 0 and r["vc_mr_single"] == 0, r
    assert r["vc_thr"] == 0 and r["vc_comp"] == 0 and r["vc_tail"] == 0, r
    ds.solve_n(B[:, :5])
    r = oa.route_stats()
    assert r["vc_mr_single"] == 1, r
    oa.vc_mrhs_k(())                                     # no group size: every column single
    X = ds.solve_n(B[:, :3])
    r = oa.route_stats()
    assert r["vc_mr_single"] == 3 and r["vc_mr_thr"] == 0 and r["vc_mr_wave"] == 0
    assert same_bits(X, ref[False][:, :3])


@pytest.mark.parametrize("row_max", [6, 12])
def test_solve_n_levels_with_outlier_rows(row_max):
    """a plan built with the outlier limit lowered to 6 / 12 entries: some levels of p7_12 run
    column by column through the single-vector code, the others through the K-column kernels,
    and the bits are the unchanged hierarchy's"""
    _, _, B, ref = setup_of("p7_12")
    oa.vc_row_max(row_max)
    ds = oa.DeviceSetup(*_coo("p7_12"))
    try:
        ds.run()
        for nrhs, flag in ((8, False), (7, True), (2, False)):
            oa.route_stats()
            X = ds.solve_n(B[:, :nrhs], remove_mean=flag)
            r = oa.route_stats()
            assert same_bits(X, ref[flag][:, :nrhs]), (row_max, nrhs, flag)
            assert r["vc_mr_comp"] > 0 and r["vc_mr_thr"] + r["vc_mr_wave"] > 0, r
        assert same_bits(ds.solve(B[:, 0]), ref[False][:, 0])
    finally:
        oa.vc_row_max(0)
        ds.close()


def test_many_solve_n_calls_queue_no_timing_events():
    """600 solve_n calls on a plan whose long-row levels fall back column by column to the
    composed products, these through the setup's event-timed lane kernel: the event pairs
    waiting to be read stay bounded (the calls' own timer is read every 256 calls), none is
    left on the setup's slots, and the bytes count the fallen-back matrices once per column"""
    L = oa.lib()
    L.amgd_test_timer_pending.restype = C.c_uint64
    _, _, B, ref = setup_of("sem_e2_N7")
    n0 = B.shape[0]
    oa.vc_row_max(16)                 # every matrix with a mean row of 32 entries is past it
    oa.spmv_sl_min(0)                 # the lane kernel at any row count, as on large levels
    oa.vc_mrhs_k((2,))
    ds = oa.DeviceSetup(*_coo("sem_e2_N7"))
    try:
        ds.run()
        oa.stats()
        oa.solve_stats()              # read what is pending
        oa.solve_n_stats()
        base = L.amgd_test_timer_pending()
        oa.route_stats()
        X = ds.solve_n(B[:, :4])      # two groups of 2
        r = oa.route_stats()
        assert r["spmv_pipe"] > 0 and r["vc_mr_comp"] > 0, r     # the timed kernel is on the path
        assert same_bits(X, ref[False][:, :4])
        by = oa.solve_n_stats()["bytes"]
        x = ds.solve(B[:, 0])
        one = oa.solve_stats()["bytes"]
        assert same_bits(x, ref[False][:, 0])
        oa.vc_row_max(0)
        whole = oa.DeviceSetup(*_coo("sem_e2_N7"))      # the same hierarchy, no level falls back
        try:
            whole.run()
            whole.solve_n(B[:, :4])
            assert oa.solve_n_stats()["bytes"] < by <= 4 * one
        finally:
            whole.close()
        oa.solve_stats()
        oa.solve_n_stats()
        assert L.amgd_test_timer_pending() == base
        seen = 0
        for k in range(600):
            assert L.amgd_solve_device_n(ds.h, ds.dxn, ds.dbn, 4, n0, 0) == 0
            seen = max(seen, L.amgd_test_timer_pending())
        assert seen - base <= 256, (base, seen)
        st = oa.solve_n_stats()       # drains the calls' own timer
        assert L.amgd_test_timer_pending() == base
        assert st["ms"] > 0
    finally:
        oa.vc_row_max(0)
        oa.spmv_sl_min(-1)
        ds.close()


# ------------------------------------------------------------------ one level, synthetic
def rand_csr(rng, rn, cn, lens, dyadic):
    """rows of the given lengths, columns ascending (repeats allowed), values dyadic or normal"""
    lens = np.minimum(np.asarray(lens, dtype=np.int64), 10 ** 9)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(ro[-1])
    row = np.repeat(np.arange(rn), lens)
    col = rng.integers(0, cn, nnz)
    o = np.lexsort((col, row))
    a = rng.integers(-16, 17, nnz) / 8.0 if dyadic else rng.standard_normal(nnz)
    return abi.Csr(rn, cn, ro, col[o].astype(np.int64), a)


def level_case(seed, nf, nc, lens_f, lens_c, dyadic, K, outlier=None):
    """(Af, W, AfP, D, BF (nf, K), XC (nc, K)); lens_f / lens_c: row lengths of Af / of W and AfP
    (callables of rng and nf); outlier: (matrix name, row, length)"""
    rng = np.random.default_rng(seed)
    lf, lw, lp = lens_f(rng, nf), lens_c(rng, nf), lens_c(rng, nf)
    if outlier:
        {"Af": lf, "W": lw, "AfP": lp}[outlier[0]][outlier[1]] = outlier[2]
    Af, W, AfP = rand_csr(rng, nf, nf, lf, dyadic), rand_csr(rng, nf, nc, lw, dyadic), rand_csr(rng, nf, nc, lp, dyadic)
    if dyadic:
        D = 2.0 ** -rng.integers(2, 5, nf)
        BF, XC = rng.integers(-8, 9, (nf, K)) / 4.0, rng.integers(-8, 9, (nc, K)) / 4.0
    else:
        D = rng.uniform(0.05, 0.3, nf)
        BF, XC = rng.standard_normal((nf, K)), rng.standard_normal((nc, K))
    return Af, W, AfP, D, BF, XC


def near(mean):
    return lambda rng, n: rng.integers(max(mean - mean // 4, 0), mean + mean // 4 + 2, n)


def exactly(mean):
    return lambda rng, n: np.full(n, mean)


def mixed(rng, n):
    """0, 1, 63, 64, 65, 129 entries among rows of 1 to 3: mean below 16"""
    lens = rng.integers(1, 4, n)
    lens[::32] = 0
    for q, v in enumerate((1, 63, 64, 65, 129)):
        lens[q + 1::32] = v
    return lens


def level_ref(case, m, rho):
    Af, W, AfP, D, BF, XC = case
    cols = [refsolve.level_up(Af, W, AfP, D, m, rho, BF[:, j], XC[:, j]) for j in range(BF.shape[1])]
    return tuple(np.stack([c[q] for c in cols], axis=1) for q in range(3))


def check_level(case, m, rho, families=FAMILIES, ref=None):
    Af, W, AfP, D, BF, XC = case
    ref = ref or level_ref(case, m, rho)
    for fam in families:
        oa.route_stats()
        got = oa.test_vc_level_n(Af, W, AfP, D, m, rho, BF, XC, fam)
        r = oa.route_stats()
        for name, g, w in zip(("xf", "bf", "c"), got, ref):
            assert same_bits(g, w), (fam, BF.shape[1], m, name, int(np.sum(g.view(np.uint64) != w.view(np.uint64))))
        if fam == "short":
            assert r["vc_mr_thr"] == m and r["vc_mr_wave"] == 0 and r["vc_mr_comp"] == 0, (fam, r)
        if fam == "long":
            assert r["vc_mr_wave"] == m and r["vc_mr_thr"] == 0 and r["vc_mr_comp"] == 0, (fam, r)
    return ref


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "general"])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 6])
def test_level_n_mixed_rows_every_m(m, dyadic, K):
    """rows of 0, 1, 63, 64, 65 and 129 entries, m = 1 .. 6, both kernel families"""
    case = level_case(100 + m, 320, 200, mixed, mixed, dyadic, K)
    check_level(case, m, 0.6, ("auto",) + FAMILIES)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nf", [1, 255, 256, 257, 4095, 4097])
def test_level_n_sizes(nf, K):
    case = level_case(nf, nf, max(1, nf // 3), near(3), near(3), False, K)
    check_level(case, 3, 0.7)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mean", [3, 15, 16, 17, 40, 200])
def test_level_n_mean_row_lengths(mean, K):
    """every row of exactly `mean` entries (15 / 16 / 17: both sides of the family switch, which
    is at a mean of 16; 16 is also the long-row tile's segment) and rows near it: the family by
    row shape, and each family forced on the other's shape"""
    nf = 300 if mean < 100 else 130
    for lens in (exactly(mean), near(mean)):
        case = level_case(mean, nf, 257, lens, lens, False, K)
        ref = check_level(case, 3, 0.5)
        Af, W, AfP, D, BF, XC = case
        oa.route_stats()
        got = oa.test_vc_level_n(Af, W, AfP, D, 3, 0.5, BF, XC, "auto")
        r = oa.route_stats()
        assert all(same_bits(g, w) for g, w in zip(got, ref))
        long_p, long_c = max(W.nnz, AfP.nnz) >= 16 * nf, Af.nnz >= 16 * nf
        assert r["vc_mr_wave"] == long_p + 2 * long_c and r["vc_mr_thr"] == 3 - r["vc_mr_wave"], (mean, r)
        if mean in (15, 16, 17) and W.nnz == mean * nf:      # every row exactly `mean` long
            assert long_p == (mean >= 16) and long_c == (mean >= 16)

def special_lens(rng, n):
    """rows of 0 entries, of the short-row chunk (2 048) and the long-row segment (16) and those
    +- 1, and one row of 4 096 entries (the longest the K-column kernels take), among rows of 3"""
    lens = rng.integers(2, 5, n)
    lens[::9] = 0
    for q, v in enumerate((2047, 2048, 2049, 15, 16, 17, 4096, 31, 32, 33)):
        lens[5 + 11 * q] = v
    return lens


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "general"])
def test_level_n_special_row_lengths(K, dyadic):
    case = level_case(5, 300, 5000, special_lens, special_lens, dyadic, K)
    Af, W, AfP = case[:3]
    for M in (Af, W, AfP):
        assert np.diff(M.row_off).max() == 4096 and np.diff(M.row_off).min() == 0
    check_level(case, 3, 0.5, ("auto",) + FAMILIES)


@pytest.mark.parametrize("K", KS)
def test_level_n_signed_zeros_and_cancellation(K):
    """-0.0 entries, rows whose products cancel exactly, -0.0 in b and x"""
    rng = np.random.default_rng(4)
    nf, nc = 96, 64
    lens = np.tile([2, 1, 0, 4], nf // 4)
    Af, W, AfP = rand_csr(rng, nf, nf, lens, True), rand_csr(rng, nf, nc, lens, True), rand_csr(rng, nf, nc, lens, True)
    XC = np.ones((nc, K))
    for j in range(K):
        XC[j % 5::5, j] = -0.0
    XC[:, K - 1] = -0.0
    for M in (W, AfP):
        for i in range(0, nf, 4):                 # rows of two entries: a and -a against equal x
            k = M.row_off[i]
            M.col[k], M.col[k + 1] = 1, 2
            M.a[k + 1] = -M.a[k]
        for i in range(1, nf, 8):                 # a single -0.0 entry
            M.a[M.row_off[i]] = -0.0
    D = np.full(nf, 0.25)
    BF = rng.integers(-4, 5, (nf, K)) / 2.0
    for j in range(K):
        BF[j % 3::3, j] = -0.0
    for m in (1, 2, 3):
        check_level((Af, W, AfP, D, BF, XC), m, 0.5)


@pytest.mark.parametrize("K", KS)
def test_level_n_columns_are_independent(K):
    """all K columns equal come out equal; a permutation of the columns permutes the results:
    a column depends on its own data only"""
    for mean in (3, 40):
        case = level_case(60 + mean, 333, 257, near(mean), near(mean), False, K)
        Af, W, AfP, D, BF, XC = case
        ref = level_ref(case, 3, 0.5)
        perm = np.roll(np.arange(K), 1)
        for fam in FAMILIES:
            got = oa.test_vc_level_n(Af, W, AfP, D, 3, 0.5, BF[:, perm], XC[:, perm], fam)
            for g, w in zip(got, ref):
                assert same_bits(g, w[:, perm]), (fam, mean)
            eqB, eqX = np.repeat(BF[:, :1], K, axis=1), np.repeat(XC[:, :1], K, axis=1)
            got = oa.test_vc_level_n(Af, W, AfP, D, 3, 0.5, eqB, eqX, fam)
            for g, w in zip(got, ref):
                for j in range(K):
                    assert same_bits(g[:, j], w[:, 0]), (fam, mean, j)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("which", ["Af", "W"])
def test_level_n_outlier_row_falls_back(which, K):
    """one 4 097-entry row: no K-column form; the level runs column by column through the
    single-vector kernels, counted by vc_mr_comp"""
    case = level_case(9, 4200, 4200, near(3), near(3), False, K, outlier=(which, 7, 4097))
    Af, W, AfP, D, BF, XC = case
    ref = level_ref(case, 2, 0.5)
    oa.route_stats()
    got = oa.test_vc_level_n(Af, W, AfP, D, 2, 0.5, BF, XC, "auto")
    r = oa.route_stats()
    for g, w in zip(got, ref):
        assert same_bits(g, w)
    assert r["vc_mr_comp"] == K and r["vc_mr_thr"] == 0 and r["vc_mr_wave"] == 0 and r["vc_comp"] > 0, r
    assert r["vc_mr_single"] == 0


# ------------------------------------------------------------------ restriction
def check_restrict(W, seed, K, want_single=False):
    rng = np.random.default_rng(seed)
    BF, BC = rng.standard_normal((W.rn, K)), rng.standard_normal((W.cn, K))
    ref = np.stack([refsolve.restrict(W, BF[:, j], BC[:, j]) for j in range(K)], axis=1)
    for fam in ("auto",) + FAMILIES:
        oa.route_stats()
        got = oa.test_vc_restrict_n(W, BF, BC, fam)
        r = oa.route_stats()
        assert same_bits(got, ref), (fam, K)
        if want_single:
            assert r["vc_mr_comp"] == K and r["vc_mr_thr"] + r["vc_mr_wave"] == 0, r
        elif fam != "auto":
            assert r["vc_mr_thr" if fam == "short" else "vc_mr_wave"] == 1 and r["vc_mr_comp"] == 0, r


@pytest.mark.parametrize("K", KS)
def test_restrict_n_shapes(K):
    rng = np.random.default_rng(8)
    # empty columns: only the first 100 of 200 are used
    W = rand_csr(rng, 300, 100, near(3)(rng, 300), False)
    W.cn = 200
    check_restrict(W, 1, K)
    # nc = 1, and nf around the block sizes
    check_restrict(rand_csr(rng, 40, 1, np.tile([1, 0], 20), False), 2, K)
    for nf in (1, 255, 256, 257, 4095, 4097):
        check_restrict(rand_csr(rng, nf, max(1, nf // 3), near(3)(rng, nf), False), nf, K)
    # long columns: 64 columns of about 190 entries each, then 7 of about 2 050 (past the chunk)
    check_restrict(rand_csr(rng, 4097, 64, near(3)(rng, 4097), False), 3, K)
    check_restrict(rand_csr(rng, 4097, 7, near(3)(rng, 4097), False), 4, K)
    # W' rows of 15 / 16 / 17 and of 4 096 entries exactly
    for n in (15, 16, 17, 4096):
        W = rand_csr(rng, n, 1, np.ones(n, dtype=np.int64), False)
        check_restrict(W, n, K)
    # mixed row lengths in W, dyadic
    check_restrict(rand_csr(rng, 320, 200, mixed(rng, 320), True), 5, K)


@pytest.mark.parametrize("K", KS)
def test_restrict_n_outlier_column_falls_back(K):
    """a column of 4 097 entries among short ones: W' has an outlier row"""
    rng = np.random.default_rng(9)
    W = rand_csr(rng, 4300, 3000, near(2)(rng, 4300), False)
    W.col[W.row_off[:4097]] = 0
    o = np.lexsort((W.col, np.repeat(np.arange(W.rn), np.diff(W.row_off))))
    W.col = W.col[o]
    assert np.bincount(W.col, minlength=W.cn).max() > 4096
    check_restrict(W, 4, K, want_single=True)


# ------------------------------------------------------------------ errors
def test_solve_n_bad_arguments():
    ds, h, B, ref = setup_of("p7_12")
    n0 = B.shape[0]
    rc, _ = ds.solve_n(B[:, :0], check=False)
    assert rc == -1
    rc, X = ds.solve_n(B[:, :2], ld=n0 - 1, check=False)
    assert rc == -1 and np.all(np.isnan(X))
    L = oa.lib()
    assert L.amgd_solve_device_n(None, None, None, 1, 1, 0) == -1
    assert L.amgd_solve_device_n(ds.h, None, ds.dbn, 1, n0, 0) == -1


def test_solve_n_rejects_partitioned_hierarchy():
    """a hierarchy built by the partitioned driver (one-rank RCCL communicator, in this
    process): -3 with and without flag bit 2, nothing allocated, nothing written"""
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
        rc, X = ds.solve_n(np.ones((n, 2)), check=False)      # allocates the test's own blocks
        assert rc == -3 and np.all(np.isnan(X))
        before = L.amgd_test_pool_inuse()
        for flags in (0, 4, 5):
            assert L.amgd_solve_device_n(ds.h, ds.dxn, ds.dbn, 2, n, flags) == -3
        assert L.amgd_test_pool_inuse() == before
    finally:
        if ds is not None:
            ds.close()
        shard.free()


def test_solve_n_out_of_hbm_recovers():
    """the cap set after a successful single solve so that the K = 8 work vectors (4 N 8
    doubles) do not fit: -2 with the reason, the pool back to its value before; with the cap
    lifted solve_n and solve give the reference bits"""
    L = oa.lib()
    L.amgd_test_hbm_cap.argtypes = [C.c_uint64]
    L.amgd_test_pool_inuse.restype = C.c_uint64
    Ai, Aj, Av = _coo("p7_12")
    ds = oa.DeviceSetup(Ai, Aj, Av)
    try:
        ds.run()
        h = ds.export()
        n0 = int(h.levels[0].n)
        B = mrhs_inputs.block(n0)[:, :8]
        ref = np.stack([refsolve.vcycle(h, B[:, j]) for j in range(8)], axis=1)
        assert same_bits(ds.solve(B[:, 0]), ref[:, 0])
        rc, _ = ds.solve_n(B, ld=n0 - 1, check=False)          # the test's own device blocks, no work
        assert rc == -1
        before = L.amgd_test_pool_inuse()
        L.amgd_test_hbm_cap(before + 2 * 8 * 8 * n0)           # two of the four vectors fit
        rc, _ = ds.solve_n(B, check=False)
        L.amgd_test_hbm_cap(0)
        assert rc == -2 and b"out of HBM" in L.amgd_error()
        assert L.amgd_test_pool_inuse() == before
        assert same_bits(ds.solve(B[:, 1]), ref[:, 1])
        assert same_bits(ds.solve_n(B), ref)
        assert same_bits(ds.solve(B[:, 2]), ref[:, 2])
    finally:
        L.amgd_test_hbm_cap(0)
        ds.close()


# ------------------------------------------------------------------ crs
def _crs_check(n, ids, Ai, Aj, Av, null_space, seed):
    L = oa.lib()
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, 3))
    X0 = np.full((n, 3), np.nan)
    hd = abi.crs_setup(L, n, ids, Ai, Aj, Av, null_space=null_space)
    assert hd is not None
    try:
        h = abi.crs_export(L, hd)
        X = abi.crs_solve_n(L, hd, B, X0=X0)
        assert same_bits(abi.crs_solve_n.b_after, B)
        Xp = abi.crs_solve_n(L, hd, B, X0=X0, ld=n + 2)
        cols = [abi.crs_solve(L, hd, B[:, j]) for j in range(3)]
        rc, _ = abi.crs_solve_n(L, hd, B, ld=n - 1, check=False)
        assert rc == -1
    finally:
        L.crs_free(hd)
    for j in range(3):
        assert same_bits(X[:, j], cols[j]) and same_bits(Xp[:, j], cols[j]), j
        assert same_bits(X[:, j], refsolve.crs_solve(h, ids, B[:, j], null_space)), j
    dead = np.asarray(ids) == 0
    assert np.all(np.isnan(X[dead])) and not np.any(np.isnan(X[~dead]))
    return X


def test_crs_solve_n_crs_test_matrix():
    """crs_test.c's 4 x 4 singular Laplacian with its ids, and with permuted ids"""
    _crs_check(4, np.array([1, 2, 3, 4]), CRS_I, CRS_J, CRS_A, 1, 1)
    ids = np.array([3, 1, 4, 2])
    _crs_check(4, ids, CRS_I, CRS_J, CRS_A, 1, 2)


def test_crs_solve_n_amgdmp_scrambled():
    """amgdmp with scrambled ids, two id-0 dofs and one dof present twice"""
    z = np.load(os.path.join(GOLD, "amgdmp.npz"))
    Ai, Aj, Av = z["in_Ai"].astype(np.int64), z["in_Aj"].astype(np.int64), z["in_Av"]
    n = int(Ai.max()) + 1
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    ids = np.concatenate([perm + 1, [0, 0, perm[5] + 1]])
    X = _crs_check(n + 3, ids, inv[Ai], inv[Aj], Av, 1, 3)
    assert same_bits(X[n + 2], X[5])
