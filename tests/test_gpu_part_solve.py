"""The V-cycle on the row-partitioned hierarchy (DESIGN.md "Solve", the partitioned part):
amgd_solve_device and crs_solve with several ranks, bit for bit against the host restatement
on the hierarchy the same run exported.  N processes share the test box's one GPU over the
host transport with the collective guard on (tests/part_solve_worker.py); one launch does one
setup and loops over the modes in-process."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import omp_amg_amd as oa
from omp_amg_amd import abi, problems, shard
import part_cases as pc
import refops
import refsolve

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(size, what, timeout=150, **env):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(size),
               PYTHONPATH=ROOT, AMGD_COMM_CHECK="1", AMGD_ARENA_GB=os.environ.get("PART_ARENA_GB", "8"),
               PS_WHAT=what, **env)
    ps = [subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "tests", "part_solve_worker.py")],
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
        raise AssertionError("\n".join(f"--- rank {r} rc={rc}\n{o[-6000:]}\n{e}" for r, (rc, o, e) in enumerate(outs)))
    res = [json.loads(o.strip().splitlines()[-1]) for _, o, _ in outs]
    for d in res:
        assert not d["bad"] and d["leak_bytes"] == 0, d
    return res


def _stats_agree(res):
    """amgd_solve_comm_stats (collectives, bytes all ranks send) is the same on every rank"""
    for d in res[1:]:
        assert d["stats"] == res[0]["stats"], (d["rank"], d["stats"], res[0]["stats"])
    return res[0]["stats"]


@pytest.mark.parametrize("size,case", [(2, "gold:p7_12"), (3, "gold:p27_8"), (4, "gold:aniso_12"),
                                       (4, "gold:sem_e2_N7"), (8, "gold:amgdmp")],
                         ids=lambda v: str(v).replace("gold:", ""))
def test_partitioned_cycle_matches_refsolve(size, case):
    """every rank's own rows of x (and, completed, every row) equal refsolve.vcycle on the
    exported hierarchy in every mode: {halo, allgather} x replication {0, default, everything} x
    {fused, cooperative, composed} x {mean, no mean}; db unchanged; the second call the same
    bits; rows of other ranks not written; nothing left on the device.  Without the feature
    amgd_solve_device returns -3.  (aniso_12 and sem_e2_N7 have levels with m = 3: two c
    exchanges; amgdmp has a null space and, on 8 ranks, ranks without rows on coarse levels.)"""
    res = _run(size, "cycle", PS_CASE=case, timeout=280)
    st = _stats_agree(res)
    # with replication 0 every cycle makes at least one collective (the worker checks it per
    # rank); everything replicated: exactly the one that completes b (plus x's for flag 2)
    for tag, (coll, _) in st.items():
        if tag.startswith("repl=0 "):
            assert coll >= 1, (tag, coll)
        if tag.startswith(f"repl={1 << 40} "):
            assert coll == 1, (tag, coll)


def test_partitioned_cycle_24_boundary_level():
    """7-point 24^3 on 2 ranks; besides the modes above the replication limit just above and
    just below level 1's slice size, so the boundary level falls on either side.  Halo mode
    sends strictly fewer bytes than allgather mode, and default replication uses strictly
    fewer collectives than replication 0"""
    res = _run(2, "cycle", PS_CASE="p7:24", PS_REPL="level1", timeout=280)
    st = _stats_agree(res)
    for k in ("fused", "composed"):
        for m in (0, 1):
            halo, allg = st[f"repl=0 halo=1 {k} mean={m}"], st[f"repl=0 halo=0 {k} mean={m}"]
            assert halo[1] < allg[1], (halo, allg)
            assert st[f"repl=-1 halo=1 {k} mean={m}"][0] < halo[0]
    lims = sorted(int(t.split()[0][5:]) for t in st if t.endswith("halo=1 fused mean=0"))
    n1 = lims[-2]                                   # 0, n1 - 1, n1, the default ... : see the worker
    a, b = st[f"repl={n1} halo=1 fused mean=0"], st[f"repl={n1 - 1} halo=1 fused mean=0"]
    assert a[0] < b[0], (a, b)                      # level 1 replicated saves its exchanges


def test_partitioned_cycle_one_rank_rccl():
    """a one-rank RCCL communicator in partitioned mode on p7_24: the partitioned plan and
    cycle on a single block (no exchange), every mode, against refsolve"""
    oa.init()
    L = oa.lib()
    import ctypes as C
    uid = C.create_string_buffer(128)
    assert L.amgd_comm_rccl_uid(uid) == 0
    assert L.amgd_comm_init_rccl(0, 1, uid.raw) == 0
    try:
        L.amgd_comm_set_partitioned(1)
        ds = oa.DeviceSetup(*problems.poisson3d(24))
        ds.run()
        h = ds.export()
        n0 = int(h.levels[0].n)
        assert ds.rows() == (0, n0)
        b = np.random.default_rng(11).standard_normal(n0)
        ref = {f: refsolve.vcycle(h, b, remove_mean=f) for f in (False, True)}
        for repl in (0, -1, 1 << 40):
            oa.vc_repl(repl)
            for halo in (1, 0):
                oa.vc_halo(halo)
                for fused, coop in ((-1, -1), (1, 1), (0, -1)):
                    oa.vc_fused(fused)
                    oa.vc_coop(coop)
                    for mean in (False, True):
                        x = ds.solve(b, remove_mean=mean, partitioned=True)
                        assert pc.diff_vec(x, ref[mean]) is None, (repl, halo, fused, mean)
                        assert pc.diff_vec(ds.b_after, b) is None
                        assert oa.solve_comm_stats() == {"collectives": 0, "bytes": 0}
        ds.close()
    finally:
        for f in (oa.vc_fused, oa.vc_coop, oa.vc_halo, oa.vc_repl):
            f(-1)
        shard.free()


def test_hier_rows_one_gpu():
    oa.init()
    ds = oa.DeviceSetup(*problems.poisson3d(6))
    ds.run()
    assert ds.rows() == (0, 216)
    # flag bit 2 (the partitioned call) changes nothing on a one-GPU hierarchy
    b = np.random.default_rng(2).standard_normal(216)
    assert pc.diff_vec(ds.solve(b, partitioned=True), ds.solve(b)) is None
    ds.close()


@pytest.mark.parametrize("size", [2, 3, 4])
def test_halo_exchange_alone(size):
    """every rank keeps its row block of a random matrix, builds the halo list and runs one
    exchange on a vector holding the truth on its own entries and a poison pattern elsewhere:
    afterwards every referenced entry holds the truth, every unreferenced entry it does not
    own still the poison.  Partition kinds even, ragged, empty and one_owner (rows and vector
    split independently), 3 seeds each, in one launch per rank count"""
    _run(size, "halo", timeout=120)


def _rand(rng, rn, cn, lens):
    M = pc.with_row_lengths(rng, rn, cn, lens)
    return abi.Csr(M.rn, M.cn, M.row_off, M.col, M.a)


@pytest.mark.parametrize("shape", ["short", "long", "mixed"])
@pytest.mark.parametrize("mode", ["thr", "coop", "composed"])
def test_mapped_restriction_kernels(shape, mode):
    """b[cmap[c]] += (W' bF)[c] on a ragged own-row set [c0, c1) of the C points, the map a
    scattered set of positions: both kernel shapes and the composed form against
    refsolve.restrict; the positions outside the map stay as they were.  More than one block of
    256 rows, odd sizes, empty rows, and rows past one LDS chunk in the long shape"""
    rng = np.random.default_rng({"short": 1, "long": 2, "mixed": 3}[shape])
    nf, nc = 1531, 777
    lens = {"short": rng.integers(0, 6, nf), "long": rng.integers(20, 60, nf),
            "mixed": np.where(rng.random(nf) < 0.02, 300, rng.integers(0, 4, nf))}[shape]
    W = _rand(rng, nf, nc, lens)
    bF = rng.standard_normal(nf)
    c0, c1 = 113, 690                                   # 577 own C rows: three blocks, the last ragged
    Wt = refops.transpose(refops.Csr(W.rn, W.cn, W.row_off, W.col, W.a))
    own = pc.block(Wt, c0, c1)
    nb = 2048
    cmap = rng.permutation(nb)[:c1 - c0]
    b = rng.standard_normal(nb)
    want = b.copy()
    bC = np.zeros(nc)
    bC[c0:c1] = b[cmap]
    want[cmap] = refsolve.restrict(W, bF, bC)[c0:c1]
    oa.vc_rw(0)
    got = oa.test_vc_restrict_map(abi.Csr(own.rn, own.cn, own.row_off, own.col, own.a), bF, b, cmap, mode)
    assert pc.diff_vec(got, want) is None, pc.diff_vec(got, want)


@pytest.mark.parametrize("size,case", [(2, "crs4"), (3, "crs4"), (2, "amgdmp"), (3, "amgdmp")])
def test_crs_solve_ranks(size, case):
    """crs_setup + crs_solve with np = 2 and 3: the 4 x 4 crs_test.c matrix and amgdmp with
    scrambled ids, id-0 dofs and dofs shared between ranks, in the partitioned and the
    replicated setup mode, against refsolve_part.crs_solve_ranks bit for bit; b unmodified; a
    second solve the same.  Without the feature crs_solve aborts."""
    _run(size, "crs", PS_CASE=case, timeout=200)
