"""Flexible GMRES on the row-partitioned hierarchy (DESIGN.md "Krylov on the row-partitioned
hierarchy"): amgd_krylov_device with flag bit 2 and amgd_crs_krylov with several ranks.  N
processes share the test box's one GPU over the host transport with the collective guard on
(tests/part_krylov_worker.py); one launch does one setup and a handful of solves, and every
yardstick is computed on the hierarchy the same run exported.  Without the feature every call
here returns -3."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import omp_amg_amd as oa
from omp_amg_amd import problems, shard
import refkrylov
import refsolve

pytestmark = pytest.mark.gpu

RTOL, MAXIT = 1e-10, 30


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(size, what, timeout=150, **env):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(size),
               PYTHONPATH=ROOT, AMGD_COMM_CHECK="1", AMGD_ARENA_GB=os.environ.get("PART_ARENA_GB", "8"),
               PK_WHAT=what, **env)
    ps = [subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "tests", "part_krylov_worker.py")],
                           env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
          for r in range(size)]
    outs = []
    for p in ps:
        try:
            o, e = p.communicate(timeout=timeout)      # every time limit ends the launch
        except subprocess.TimeoutExpired:
            for q in ps:
                q.kill()
            raise
        outs.append((p.returncode, o, e[-3000:]))
    if any(rc != 0 for rc, _, _ in outs):
        for q in ps:
            q.kill()
        raise AssertionError("\n".join(f"--- rank {r} rc={rc}\n{o[-6000:]}\n{e}" for r, (rc, o, e) in enumerate(outs)))
    res = [json.loads(o.strip().splitlines()[-1]) for _, o, _ in outs]
    for d in res:
        assert not d["bad"] and d["leak_bytes"] == 0, d
    return res


@pytest.mark.parametrize("size,case", [(2, "gold:p7_12"), (3, "gold:p27_8"), (4, "gold:aniso_12"), (8, "gold:amgdmp")],
                         ids=lambda v: str(v).replace("gold:", ""))
def test_partitioned_krylov(size, case):
    """b = A x*, rtol 1e-10, maxit 30.  Ordered: the own rows of x, info and hist equal
    refkrylov.fgmres bit for bit with restart 30 and 5 in halo and allgather mode with
    replication 0 and default, with a guess, with maxit 4 (rc 1), with bit 3 (every row) and
    in a second call; db unchanged; rows of other ranks not written
    without bit 3; 0 device bytes left after close().  Fused: rc 0, its within one of the
    ordered count, the host-recomputed residual at most rtol (1 + 1e-3) ||b||, two runs the same
    bits, info / hist / x identical on all ranks, only multi-dot launches, rank-order combines,
    and amgd_krylov_comm_stats equal to the documented formula on every rank.  The workspace of
    the first m = 30 call is under half of the one-GPU (2 m + 4) n0 8 bytes on 4 ranks.
    (aniso_12 has levels with m = 3; amgdmp has 49 rows, a null space and, on 8 ranks, ranks
    without coarse rows.)"""
    res = _run(size, "solve", PK_CASE=case, timeout=280)
    for d in res[1:]:
        assert d["stats"] == res[0]["stats"], (d["rank"], d["stats"], res[0]["stats"])
    if size == 4:
        for d in res:
            print("rank", d["rank"], "workspace growth", d["ws_growth"], "one-GPU workspace", d["ws_one_gpu"])
            assert d["ws_growth"] < d["ws_one_gpu"] / 2, d


@pytest.mark.parametrize("size", [2, 3, 4])
def test_rank_order_combine_alone(size):
    """test_kry_mdot_ranks and test_kry_norm_ranks: every partition kind, n = 1, 257, 4097,
    nb = 1, 16, 17.  The one-GPU hooks' values on every rank's slice, gathered and added in rank
    order in numpy, are the hooks' bits, and the sums lie within test_kernel_hooks' bound
    n u / (1 - n u) sum|v_i w_i| of the exact sum"""
    _run(size, "combine", timeout=150)


@pytest.mark.parametrize("size", [2, 3, 4])
def test_partitioned_product_alone(size):
    """test_kry_spmv_part on random 301 x 257 matrices, every partition kind, 3 seeds: the
    operand holds the truth on the own entries and a poison pattern elsewhere; the own rows of
    the product equal refsolve.apply_M bit for bit, the referenced entries were fetched and the
    unreferenced foreign entries still hold the poison"""
    _run(size, "product", timeout=120)


@pytest.mark.parametrize("size,case", [(2, "crs4"), (3, "crs4"), (2, "amgdmp"), (3, "amgdmp")])
def test_crs_krylov_ranks(size, case):
    """crs_setup + amgd_crs_krylov with np = 2 and 3 in the partitioned and the replicated setup
    mode, ordered, bit for bit against the rank-aware restatement (refsolve_part's assembly,
    refkrylov.fgmres); with a guess that differs between the ranks sharing an id; b unmodified;
    id-0 dofs untouched"""
    _run(size, "crs", PK_CASE=case, timeout=200)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def test_one_rank_rccl_matches_one_gpu():
    """a one-rank RCCL communicator in partitioned mode on 7-point 24^3: the fused partitioned
    x, info and hist equal the one-GPU fused solve of the same matrix bit for bit, the ordered
    ones refkrylov; amgd_krylov_comm_stats is 0 collectives; without bit 2 the call still
    returns -3"""
    oa.init()
    L = oa.lib()
    Ai, Aj, Av = problems.poisson3d(24)
    one = oa.DeviceSetup(Ai, Aj, Av)
    one.run()
    h1 = one.export()
    n0 = int(h1.levels[0].n)
    xs = np.random.default_rng(5).standard_normal(n0)
    b = refsolve.csr_matvec(h1.levels[0].A, xs)
    want = {m: one.krylov(b, rtol=RTOL, restart=m, maxit=MAXIT) for m in (30, 5)}
    one.close()
    uid = C.create_string_buffer(128)
    assert L.amgd_comm_rccl_uid(uid) == 0
    assert L.amgd_comm_init_rccl(0, 1, uid.raw) == 0
    ds = None
    try:
        L.amgd_comm_set_partitioned(1)
        ds = oa.DeviceSetup(Ai, Aj, Av)
        ds.run()
        h = ds.export()
        assert ds.rows() == (0, n0)
        x, info, _ = ds.krylov(b, check=False)
        assert info["rc"] == -3 and np.all(np.isnan(x))
        for m in (30, 5):
            for complete in (False, True):
                x, info, hist = ds.krylov(b, rtol=RTOL, restart=m, maxit=MAXIT, partitioned=True, complete=complete)
                assert info == want[m][1], (info, want[m][1])
                assert same_bits(x, want[m][0]) and same_bits(hist, want[m][2])
                assert same_bits(ds.b_after, b)
                assert oa.krylov_comm_stats() == {"collectives": 0, "bytes": 0}
        ref = refkrylov.fgmres(h, b, rtol=RTOL, restart=5, maxit=MAXIT)
        x, info, hist = ds.krylov(b, rtol=RTOL, restart=5, maxit=MAXIT, ordered=True, partitioned=True)
        assert same_bits(x, ref["x"]) and same_bits(hist, np.array(ref["hist"]))
        assert all(same_bits(np.float64(info[k]), np.float64(ref[k])) for k in
                   ("rc", "its", "restarts", "cycles", "converged", "bnorm", "r0", "resid")), (info, ref)
        assert oa.krylov_comm_stats() == {"collectives": 0, "bytes": 0}
    finally:
        if ds is not None:
            ds.close()
        shard.free()


def test_flag_bits_change_nothing_on_one_gpu():
    oa.init()
    ds = oa.DeviceSetup(*problems.poisson3d(8))
    ds.run()
    h = ds.export()
    b = refsolve.csr_matvec(h.levels[0].A, np.random.default_rng(5).standard_normal(512))
    a = ds.krylov(b, rtol=RTOL, maxit=MAXIT)
    c = ds.krylov(b, rtol=RTOL, maxit=MAXIT, partitioned=True, complete=True)
    assert same_bits(a[0], c[0]) and a[1] == c[1] and same_bits(a[2], c[2])
    ds.close()
