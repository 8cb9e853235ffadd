"""Inputs shared by tests/test_solve_mrhs_cpu.py and tests/test_gpu_solve_mrhs.py: the block of
right-hand sides the multi-RHS solve is checked on."""
import numpy as np

NCOLS = 11
ZERO_COL = 3          # all +0.0
TINY_COL = 6          # +0.0, -0.0 and denormals of both signs
CASES = ["amgdmp", "aniso_12", "sem_e2_N7", "p27_8", "p7_12", "p7_24"]


def block(n0, seed=23):
    """(n0, 11): normal columns, one all-zero column, one of mixed +-0.0 and denormals"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n0, NCOLS))
    B[:, ZERO_COL] = 0.0
    kind = rng.integers(0, 4, n0)
    tiny = rng.integers(1, 1 << 20, n0).astype(np.float64) * 5e-324     # denormals
    B[:, TINY_COL] = np.where(kind == 0, 0.0, np.where(kind == 1, -0.0, np.where(kind == 2, tiny, -tiny)))
    return B
