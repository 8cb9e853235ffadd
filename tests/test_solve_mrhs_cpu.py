"""CPU side of the multi-RHS solve's tests: the yardstick for a block is tests/refsolve.py per
column, so the block's special columns (all zero; +-0.0 and denormals) must be inputs the
restatement handles -- it terminates and gives no NaN or infinity on every golden fixture the
GPU test uses (p7_24 has no golden file: the GPU test holds it to the single-vector solve)."""
import os

import numpy as np
import pytest

from conftest import GOLD
from omp_amg_amd import parity
import mrhs_inputs
import refsolve


def test_block_columns():
    B = mrhs_inputs.block(500)
    assert B.shape == (500, mrhs_inputs.NCOLS)
    z, t = B[:, mrhs_inputs.ZERO_COL], B[:, mrhs_inputs.TINY_COL]
    assert not z.any() and not np.signbit(z).any()
    assert np.signbit(t).any() and (~np.signbit(t)).any() and (t == 0).any()
    tiny = t[t != 0]
    assert len(tiny) and np.abs(tiny).max() < np.finfo(float).tiny       # denormals only
    assert same(mrhs_inputs.block(500), B)                                 # deterministic


def same(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


@pytest.mark.parametrize("case", [c for c in mrhs_inputs.CASES if c != "p7_24"])
def test_refsolve_on_special_columns(case):
    h = parity.from_npz(np.load(os.path.join(GOLD, case + ".npz")))
    n0 = int(h.levels[0].n)
    B = mrhs_inputs.block(n0)
    for j in (mrhs_inputs.ZERO_COL, mrhs_inputs.TINY_COL):
        for flag in (False, True):
            x = refsolve.vcycle(h, B[:, j], remove_mean=flag)
            assert x.shape == (n0,) and np.all(np.isfinite(x)), (case, j, flag)
    # a zero right-hand side gives a zero cycle
    assert not refsolve.vcycle(h, B[:, mrhs_inputs.ZERO_COL]).any()
    # and a normal column is no degenerate input
    assert np.abs(refsolve.vcycle(h, B[:, 0])).max() > 0
