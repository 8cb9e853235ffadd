"""Host restatements for the partitioned solve (tests/test_gpu_part_solve.py,
tests/test_part_solve_cpu.py; DESIGN.md "Solve", the partitioned part), beside tests/refsolve.py:

  crs_solve_ranks  crs_solve on several ranks: every rank's partial sums g_r (ascending local
                   index from +0), the assembled b = +0 + g_0 + g_1 + ... in rank order, one
                   cycle, x to every local dof of every rank
  halo_lists       which entries of a vector a rank's rows reference and do not own, per owner
"""
from __future__ import annotations

import numpy as np

import refsolve


def partial_sums(n0, ids, b):
    """g_r of one rank: b of its local dofs summed per global id in ascending local index from +0"""
    ids = np.asarray(ids, dtype=np.int64)
    b = np.asarray(b, dtype=np.float64)
    g = np.zeros(n0)
    for k in range(len(ids)):
        if ids[k]:
            g[ids[k] - 1] = g[ids[k] - 1] + b[k]
    return g


def crs_solve_ranks(h, ids, b, null_space, x0=None):
    """ids, b (and x0): one array per rank.  Returns x per rank: the cycle's x at every local dof,
    id 0 untouched (x0's value, NaN where x0 is not given)"""
    n0 = int(h.levels[0].n)
    g = np.zeros(n0)
    for r in range(len(ids)):
        g = g + partial_sums(n0, ids[r], b[r])
    xg = refsolve.vcycle(h, g, remove_mean=bool(null_space))
    out = []
    for r in range(len(ids)):
        idr = np.asarray(ids[r], dtype=np.int64)
        x = np.full(len(idr), np.nan) if x0 is None else np.array(x0[r], dtype=np.float64)
        live = idr != 0
        x[live] = xg[idr[live] - 1]
        out.append(x)
    return out


def halo_lists(cols, vsplit, me):
    """cols: the column indices of rank me's rows; vsplit: the owners' split of the vector they
    index.  Returns {owner: ascending distinct indices} of the referenced entries other ranks own"""
    vsplit = np.asarray(vsplit, dtype=np.int64)
    u = np.unique(np.asarray(cols, dtype=np.int64))
    u = u[(u < vsplit[me]) | (u >= vsplit[me + 1])]
    own = np.searchsorted(vsplit, u, side="right") - 1
    # an empty range shares its start with the next one: the owner is the last rank starting there
    return {int(p): u[own == p] for p in np.unique(own)}
