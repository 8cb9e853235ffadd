"""The host restatements the partitioned-solve GPU tests compare with (tests/refsolve_part.py):
crs_solve_ranks on one rank is refsolve.crs_solve; splitting the dofs over ranks changes the
assembled b only through the stated rank-order sum; the halo-list model agrees with a
brute-force statement on every partition kind of tests/part_cases.py."""
import os

import numpy as np
import pytest

from conftest import GOLD
from omp_amg_amd import parity
import part_cases as pc
import refsolve
import refsolve_part


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _hier(name):
    return parity.from_npz(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.mark.parametrize("name,null", [("p7_4", 0), ("amgdmp", 1)])
def test_one_rank_is_crs_solve(name, null):
    h = _hier(name)
    n = int(h.levels[0].n)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    ids = np.concatenate([perm + 1, [0, perm[2] + 1]])
    b = rng.standard_normal(n + 2)
    x0 = np.full(n + 2, 42.0)
    want = refsolve.crs_solve(h, ids, b, null, x0=x0)
    got = refsolve_part.crs_solve_ranks(h, [ids], [b], null, x0=[x0])
    assert len(got) == 1 and np.array_equal(bits(got[0]), bits(want))
    assert got[0][n] == 42.0


def test_ranks_sum_in_rank_order():
    """a dof shared by three ranks: b = ((0 + g_0) + g_1) + g_2 with values whose sum depends
    on the order, and every rank gets the same x at the shared dof"""
    h = _hier("p7_4")
    n = int(h.levels[0].n)
    ids = [np.array([1, 2]), np.array([2, 1]), np.array([1, 0])]
    b = [np.array([1e16, 3.0]), np.array([0.5, 1.0]), np.array([-1e16, 9.0])]
    g = np.zeros(n)
    g[0] = ((0.0 + 1e16) + 1.0) + -1e16
    g[1] = (0.0 + 3.0) + 0.5
    xg = refsolve.vcycle(h, g)
    got = refsolve_part.crs_solve_ranks(h, ids, b, 0)
    assert g[0] != (1e16 + -1e16) + 1.0            # the order matters for these values
    assert np.array_equal(bits(got[0]), bits(xg[[0, 1]]))
    assert np.array_equal(bits(got[1]), bits(xg[[1, 0]]))
    assert bits(got[2][:1])[0] == bits(xg[:1])[0] and np.isnan(got[2][1])


@pytest.mark.parametrize("N,kind", [(N, k) for N in (2, 3, 4) for k in pc.KINDS])
def test_halo_lists_match_brute_force(N, kind):
    for seed in range(3):
        rng = np.random.default_rng(50 + seed)
        rn, cn = 41, 53
        M = pc.with_row_lengths(rng, rn, cn, rng.integers(0, 7, rn))
        rs, vs = pc.split(kind, rn, N, seed), pc.split(kind, cn, N, seed + 7)
        for me in range(N):
            cols = M.col[M.row_off[rs[me]]:M.row_off[rs[me + 1]]]
            got = refsolve_part.halo_lists(cols, vs, me)
            want = {}
            for j in range(cn):
                o = pc.owner_of(vs, j)
                if o != me and any(int(c) == j for c in cols):
                    want.setdefault(o, []).append(j)
            assert sorted(got) == sorted(want)
            for o in want:
                assert got[o].tolist() == want[o]
                assert vs[o] <= min(want[o]) and max(want[o]) < vs[o + 1]
