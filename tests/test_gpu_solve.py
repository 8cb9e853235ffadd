"""The V-cycle on the device-resident hierarchy (amgd_solve_device, crs_solve, the level
hooks) against the host restatement tests/refsolve.py -- bit for bit, on every path: fused
and composed kernels, the one-workgroup tail on and off, every row shape."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD
import omp_amg_amd as oa
from omp_amg_amd import abi, problems
import refsolve

pytestmark = pytest.mark.gpu

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
        f(-1)                      # the shipped routing; tests of the cooperative kernels turn them on
    oa.vc_rw(0)
    yield
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
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
    """one setup per case for the module: (DeviceSetup, exported hierarchy, b, x per flag)"""
    if case not in _SETUPS:
        ds = oa.DeviceSetup(*_coo(case))
        ds.run()
        h = ds.export()
        b = np.random.default_rng(11).standard_normal(int(h.levels[0].n))
        ref = {f: refsolve.vcycle(h, b, remove_mean=f) for f in (False, True)}
        _SETUPS[case] = (ds, h, b, ref)
    return _SETUPS[case]


CASES = ["amgdmp", "aniso_12", "sem_e2_N7", "p27_8", "p7_12", "p7_24"]


@pytest.mark.parametrize("case", CASES)
def test_solve_matches_refsolve(case):
    """x = one cycle of the exported hierarchy, bit for bit: the default routing (long rows
    composed), the cooperative kernels on, and composed; tail on and off, with and without the
    mean; a second call gives the same bits; db is unchanged"""
    ds, h, b, ref = setup_of(case)
    if case == "amgdmp":
        assert h.nullspace == 1 and int(h.levels[0].m) == 2
    if case in ("aniso_12", "sem_e2_N7"):
        assert int(h.levels[0].m) == 3
    for fused, coop in ((1, -1), (1, 1), (0, -1)):
        for tail in (-1, 0):
            oa.vc_fused(fused)
            oa.vc_coop(coop)
            oa.vc_tail(tail)
            for flag in (bool(h.nullspace), not h.nullspace):
                x = ds.solve(b, remove_mean=flag)
                assert same_bits(x, ref[flag]), (case, fused, coop, tail, flag, np.abs(x - ref[flag]).max())
                assert same_bits(ds.b_after, b)
            x2 = ds.solve(b, remove_mean=bool(h.nullspace))
            assert same_bits(x2, ref[bool(h.nullspace)])


def test_solve_routes():
    """p7_24: the fine levels run the thread-per-row kernels and the coarse ones the tail;
    composed and tail-off runs take neither"""
    ds, h, b, ref = setup_of("p7_24")
    assert int(h.levels[0].n) == 24 ** 3
    oa.route_stats()
    ds.solve(b)
    r = oa.route_stats()
    assert r["vc_thr"] > 0 and r["vc_tail"] == 1
    oa.vc_fused(0)
    oa.vc_tail(0)
    ds.solve(b)
    r = oa.route_stats()
    assert r["vc_thr"] == 0 and r["vc_wave"] == 0 and r["vc_tail"] == 0 and r["vc_comp"] > 0
    st = oa.solve_stats()
    assert st["cycles"] >= 2 and st["ms"] > 0 and st["bytes"] > 12 * h.levels[0].Af.nnz


def test_tail_row_limit():
    """p7_12's level 1 has 788 positions: a limit of 788 puts it in the tail, 787 does not
    (one more level of per-level launches); the bits are the same"""
    ds, h, b, ref = setup_of("p7_12")
    n1 = int(h.levels[1].n)
    counts = {}
    for rows in (n1, n1 - 1, 1024, 0):
        oa.vc_tail(rows)
        oa.route_stats()
        assert same_bits(ds.solve(b), ref[False]), rows
        r = oa.route_stats()
        counts[rows] = r["vc_thr"] + r["vc_wave"] + r["vc_comp"]
        assert r["vc_tail"] == (1 if rows else 0)
    assert counts[n1] == counts[1024] < counts[n1 - 1] < counts[0]


@pytest.mark.parametrize("case", ["p7_10", "p7_11"])
def test_tail_on_either_side_of_1024_rows(case):
    """p7_10 has 1 000 rows, so a tail of up to 1 024 positions takes the whole hierarchy;
    p7_11 has 1 331, so its level 0 stays outside: tail on gives the bits of tail off"""
    ds, h, b, ref = setup_of(case)
    n0, n1 = int(h.levels[0].n), int(h.levels[1].n)
    assert (n0 <= 1024) == (case == "p7_10") and n1 <= 1024
    got, work = {}, {}
    for rows in (1024, 0):
        oa.vc_tail(rows)
        oa.route_stats()
        got[rows] = ds.solve(b)
        r = oa.route_stats()
        work[rows] = r["vc_thr"] + r["vc_wave"] + r["vc_comp"]
        assert r["vc_tail"] == (1 if rows else 0)
    assert same_bits(got[1024], got[0]) and same_bits(got[0], ref[False])
    if case == "p7_10":
        assert work[1024] == 0                      # every level inside the one workgroup
    else:
        assert 0 < work[1024] < work[0]             # level 0 by its own kernels


def test_many_cycles_queue_no_timing_events():
    """600 composed cycles whose long-row products take the setup's event-timed lane kernel:
    the event pairs waiting to be read stay bounded (the cycles' own timer is read every 256
    cycles) and none is left on the setup's slots"""
    L = oa.lib()
    L.amgd_test_timer_pending.restype = C.c_uint64
    ds, h, b, ref = setup_of("sem_e2_N7")
    oa.vc_fused(0)
    oa.vc_tail(0)
    oa.spmv_sl_min(0)                 # the lane kernel at any row count, as on large levels
    try:
        oa.stats()
        oa.solve_stats()              # reads what is pending
        base = L.amgd_test_timer_pending()
        oa.route_stats()
        x = ds.solve(b)
        assert oa.route_stats()["spmv_pipe"] > 0      # the timed kernel is on the path
        assert same_bits(x, ref[False])
        seen = 0
        for k in range(600):
            assert L.amgd_solve_device(ds.h, ds.dx, ds.db, 0) == 0
            seen = max(seen, L.amgd_test_timer_pending())
        assert seen - base <= 256, (base, seen)
        st = oa.solve_stats()         # drains the cycles' own timer
        assert L.amgd_test_timer_pending() == base
        assert st["ms"] > 0
    finally:
        oa.spmv_sl_min(-1)


def test_solve_rejects_partitioned_hierarchy():
    """a hierarchy built by the partitioned driver (one-rank RCCL communicator, in this
    process): -3, and nothing is allocated"""
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
        rc, x = ds.solve(np.ones(n), check=False)
        assert rc == -3 and np.all(np.isnan(x))
        assert L.amgd_test_pool_inuse() == before
    finally:
        if ds is not None:
            ds.close()
        shard.free()


def test_solve_out_of_hbm_recovers():
    """a cap below the plan's need: -2 with the reason, the pool back to its value before,
    and the next solve right"""
    L = oa.lib()
    L.amgd_test_hbm_cap.argtypes = [C.c_uint64]
    L.amgd_test_pool_inuse.restype = C.c_uint64
    Ai, Aj, Av = _coo("p7_12")
    ds = oa.DeviceSetup(Ai, Aj, Av)
    try:
        ds.run()
        h = ds.export()
        b = np.random.default_rng(11).standard_normal(int(h.levels[0].n))
        ds.vectors(len(b))
        before = L.amgd_test_pool_inuse()
        L.amgd_test_hbm_cap(before + 16384)          # the plan's W' alone needs far more
        rc, _ = ds.solve(b, check=False)
        L.amgd_test_hbm_cap(0)
        assert rc == -2 and b"out of HBM" in L.amgd_error()
        assert L.amgd_test_pool_inuse() == before
        assert same_bits(ds.solve(b), refsolve.vcycle(h, b))
    finally:
        L.amgd_test_hbm_cap(0)
        ds.close()


def test_solve_rejects_empty_hierarchy():
    L = oa.lib()
    assert L.amgd_solve_device(None, None, None, 0) == -1


# ------------------------------------------------------------------ crs_solve
def test_crs_solve_crs_test_matrix():
    """crs_test.c on one rank: the 4 x 4 singular Laplacian, null_space = 1, b = id - mean"""
    L = oa.lib()
    ids = np.array([1, 2, 3, 4])
    b = ids - 2.5
    hd = abi.crs_setup(L, 4, ids, CRS_I, CRS_J, CRS_A, null_space=1)
    assert hd is not None
    try:
        h = abi.crs_export(L, hd)
        x = abi.crs_solve(L, hd, b)
        assert same_bits(abi.crs_solve.b_after, b)
        x2 = abi.crs_solve(L, hd, b)
        L.crs_stats(hd)
    finally:
        L.crs_free(hd)
    want = refsolve.crs_solve(h, ids, b, 1)
    assert same_bits(x, want) and same_bits(x2, want)
    raw = refsolve.vcycle(h, b, remove_mean=False)
    # x_i - avg rounds each entry once and avg = fl(fl(1/n) * sum) carries two roundings more
    assert abs(refsolve.seq_sum(x)) <= 4 * len(x) * np.finfo(float).eps * np.abs(raw).max()


def test_crs_solve_amgdmp_scrambled():
    """amgdmp as a local matrix with scrambled ids, two id-0 dofs and one dof present twice
    (its b in two parts): crs_solve against the restatement, id-0 entries of x untouched"""
    z = np.load(os.path.join(GOLD, "amgdmp.npz"))
    Ai, Aj, Av = z["in_Ai"].astype(np.int64), z["in_Aj"].astype(np.int64), z["in_Av"]
    n = int(Ai.max()) + 1
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    ids = np.concatenate([perm + 1, [0, 0, perm[5] + 1]])    # local n, n+1: no dofs; n+2: dof 5 again
    b = rng.standard_normal(n + 3)
    L = oa.lib()
    hd = abi.crs_setup(L, n + 3, ids, inv[Ai], inv[Aj], Av, null_space=1)
    assert hd is not None
    try:
        h = abi.crs_export(L, hd)
        x = abi.crs_solve(L, hd, b, x0=np.full(n + 3, 42.0))
        assert same_bits(abi.crs_solve.b_after, b)
    finally:
        L.crs_free(hd)
    want = refsolve.crs_solve(h, ids, b, 1, x0=np.full(n + 3, 42.0))
    assert same_bits(x, want)
    assert x[n] == 42.0 and x[n + 1] == 42.0 and x[n + 2] == x[5]
    g = x[:n]
    raw = np.abs(refsolve.crs_solve(h, ids, b, 0, x0=np.zeros(n + 3))).max()
    assert abs(refsolve.seq_sum(g)) <= 4 * n * np.finfo(float).eps * raw


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


def level_case(seed, nf, nc, lens_f, lens_c, dyadic, outlier=None):
    """(Af, W, AfP, D, bf, xc); lens_f / lens_c: row lengths of Af / of W and AfP (callables of
    rng and nf); outlier: (matrix name, row, length)"""
    rng = np.random.default_rng(seed)
    lf, lw, lp = lens_f(rng, nf), lens_c(rng, nf), lens_c(rng, nf)
    if outlier:
        {"Af": lf, "W": lw, "AfP": lp}[outlier[0]][outlier[1]] = outlier[2]
    Af, W, AfP = rand_csr(rng, nf, nf, lf, dyadic), rand_csr(rng, nf, nc, lw, dyadic), rand_csr(rng, nf, nc, lp, dyadic)
    if dyadic:
        D = 2.0 ** -rng.integers(2, 5, nf)
        bf, xc = rng.integers(-8, 9, nf) / 4.0, rng.integers(-8, 9, nc) / 4.0
    else:
        D = rng.uniform(0.05, 0.3, nf)
        bf, xc = rng.standard_normal(nf), rng.standard_normal(nc)
    return Af, W, AfP, D, bf, xc


def near(mean):
    return lambda rng, n: rng.integers(max(mean - mean // 4, 0), mean + mean // 4 + 2, n)


def mixed(rng, n):
    """0, 1, 63, 64, 65, 129 entries among rows of 1 to 3: mean below 16"""
    lens = rng.integers(1, 4, n)
    lens[::32] = 0
    for q, v in enumerate((1, 63, 64, 65, 129)):
        lens[q + 1::32] = v
    return lens


def check_level(case, m, rho, modes, want_routes=None):
    Af, W, AfP, D, bf, xc = case
    ref = refsolve.level_up(Af, W, AfP, D, m, rho, bf, xc)
    for mode in modes:
        oa.route_stats()
        got = oa.test_vc_level(Af, W, AfP, D, m, rho, bf, xc, mode)
        r = oa.route_stats()
        for name, g, w in zip(("xf", "bf", "c"), got, ref):
            assert same_bits(g, w), (mode, m, name, int(np.sum(g.view(np.uint64) != w.view(np.uint64))))
        if want_routes and mode in want_routes:
            for k, positive in want_routes[mode].items():
                assert (r[k] > 0) == positive, (mode, k, r)


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "general"])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 6])
def test_level_mixed_rows_every_m(m, dyadic):
    """rows of 0, 1, 63, 64, 65 and 129 entries, m = 1 .. 6, thread-per-row kernels, the tail
    kernel and the composed path"""
    case = level_case(100 + m, 320, 200, mixed, mixed, dyadic)
    check_level(case, m, 0.6, ("composed", "fused", "tail"),
                {"fused": {"vc_thr": True, "vc_wave": False, "vc_comp": False},
                 "composed": {"vc_thr": False, "vc_wave": False, "vc_comp": True},
                 "tail": {"vc_tail": True}})


@pytest.mark.parametrize("nf", [1, 255, 4095, 4097])
def test_level_sizes(nf):
    case = level_case(nf, nf, max(1, nf // 3), near(3), near(3), False)
    check_level(case, 3, 0.7, ("composed", "fused"), {"fused": {"vc_thr": True, "vc_comp": False}})


@pytest.mark.parametrize("rw", [0, 4, 16, 64])
@pytest.mark.parametrize("mean", [40, 200])
def test_level_long_rows_cooperative(mean, rw):
    """mean row 40 and 200: the cooperative kernels (every rows-per-wavefront shape); with
    them switched off the composed path"""
    oa.vc_coop(1)
    oa.vc_rw(rw)
    case = level_case(mean + rw, 600, 400, near(mean), near(mean), False)
    check_level(case, 3, 0.5, ("composed", "fused", "tail"),
                {"fused": {"vc_wave": True, "vc_thr": False, "vc_comp": False}})
    if rw == 0:
        for off in (0, -1):                       # switched off, and the shipped default
            oa.vc_coop(off)
            check_level(case, 3, 0.5, ("fused",), {"fused": {"vc_wave": False, "vc_comp": True}})


def test_level_cooperative_mixed_lengths_and_m():
    """the cooperative form on rows of 0 .. 129 entries among rows of 30 (rounds that end inside
    a segment, empty rows inside a wavefront's block), m = 1, 2, 6, nf no multiple of the block"""
    def lens(rng, n):
        v = np.full(n, 30)
        v[::7] = mixed(rng, n)[::7]
        return v
    oa.vc_coop(1)
    for m in (1, 2, 6):
        for rw in (4, 16, 64):
            oa.vc_rw(rw)
            case = level_case(7 * m + rw, 333, 257, lens, lens, m == 2)
            check_level(case, m, 0.4, ("composed", "fused"), {"fused": {"vc_wave": True, "vc_comp": False}})


def test_level_mean3_thread_mean40_wave():
    """mean row 3, 40 and 200 with an outlier: the thread, cooperative and composed forms each
    run where they should"""
    oa.vc_coop(1)
    a = level_case(1, 500, 300, near(3), near(3), False)
    check_level(a, 2, 0.5, ("fused",), {"fused": {"vc_thr": True, "vc_wave": False, "vc_comp": False}})
    b = level_case(2, 500, 300, near(40), near(3), False)        # Af long, W / AfP short
    check_level(b, 2, 0.5, ("fused",), {"fused": {"vc_thr": True, "vc_wave": True, "vc_comp": False}})


@pytest.mark.parametrize("which", ["Af", "W"])
def test_level_outlier_row_takes_composed(which):
    """one 5 000-entry row among rows of 3: that matrix's product runs composed, the other stays fused"""
    case = level_case(9, 5200, 5200, near(3), near(3), False, outlier=(which, 7, 5000))
    want = {"vc_comp": True, "vc_thr": True, "vc_wave": False}
    check_level(case, 2, 0.5, ("composed", "fused"), {"fused": want})


def test_level_signed_zeros_and_cancellation():
    """-0.0 entries, rows whose products cancel exactly, -0.0 in b and x"""
    rng = np.random.default_rng(4)
    nf, nc = 96, 64
    lens = np.tile([2, 1, 0, 4], nf // 4)
    Af, W, AfP = rand_csr(rng, nf, nf, lens, True), rand_csr(rng, nf, nc, lens, True), rand_csr(rng, nf, nc, lens, True)
    xc = np.ones(nc)
    xc[::5] = -0.0
    for M in (W, AfP):
        for i in range(0, nf, 4):                 # rows of two entries: a and -a against equal x
            k = M.row_off[i]
            M.col[k], M.col[k + 1] = 1, 2
            M.a[k + 1] = -M.a[k]
        for i in range(1, nf, 8):                 # a single -0.0 entry
            M.a[M.row_off[i]] = -0.0
    D = np.full(nf, 0.25)
    bf = rng.integers(-4, 5, nf) / 2.0
    bf[::3] = -0.0
    for m in (1, 2, 3):
        check_level((Af, W, AfP, D, bf, xc), m, 0.5, ("composed", "fused", "tail"))


def test_tail_kernel_at_its_row_limit():
    """a level of exactly 1 024 positions runs in the one-workgroup kernel; 1 025 is refused"""
    case = level_case(21, 700, 324, near(5), near(4), False)
    check_level(case, 3, 0.5, ("composed", "tail"), {"tail": {"vc_tail": True}})
    case = level_case(22, 700, 325, near(5), near(4), False)
    with pytest.raises(RuntimeError):
        oa.test_vc_level(*case[:4], 3, 0.5, case[4], case[5], "tail")


# ------------------------------------------------------------------ restriction
def check_restrict(W, seed, want=None):
    rng = np.random.default_rng(seed)
    bF, bC = rng.standard_normal(W.rn), rng.standard_normal(W.cn)
    ref = refsolve.restrict(W, bF, bC)
    for fused in (False, True):
        oa.route_stats()
        got = oa.test_vc_restrict(W, bF, bC, fused)
        r = oa.route_stats()
        assert same_bits(got, ref), fused
        if fused and want:
            for k, positive in want.items():
                assert (r[k] > 0) == positive, (k, r)


def test_restrict_shapes():
    rng = np.random.default_rng(8)
    # empty columns: only the first 100 of 200 are used
    W = rand_csr(rng, 300, 100, near(3)(rng, 300), False)
    W.cn = 200
    check_restrict(W, 1, {"vc_thr": True})
    # nc = 1
    W = rand_csr(rng, 40, 1, np.tile([1, 0], 20), False)
    check_restrict(W, 2)
    # long columns: 64 columns of about 190 entries each (cooperative), every rows-per-wavefront shape
    W = rand_csr(rng, 4097, 64, near(3)(rng, 4097), False)
    oa.vc_coop(1)
    for rw in (0, 4, 16, 64):
        oa.vc_rw(rw)
        check_restrict(W, 3, {"vc_wave": True, "vc_comp": False})
    oa.vc_rw(0)
    oa.vc_coop(-1)
    # a column of 5 000 entries among short ones: composed
    lens = near(2)(rng, 5200)
    W = rand_csr(rng, 5200, 4000, lens, False)
    W.col[W.row_off[:5000]] = 0
    o = np.lexsort((W.col, np.repeat(np.arange(W.rn), np.diff(W.row_off))))
    W.col = W.col[o]
    check_restrict(W, 4, {"vc_comp": True, "vc_thr": False, "vc_wave": False})
