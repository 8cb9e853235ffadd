"""The multi-RHS Krylov solver's contract without a GPU: the public header declares its entry
points, and the shared inputs (tests/krylov_mrhs_inputs.py) make the columns' solves end after
different numbers of iterations under the host restatement -- which is what keeps the route
assertions of tests/test_gpu_krylov_mrhs.py (slots handed on, columns at different inner
indices) from being vacuous."""
import pytest

import krylov_mrhs_inputs as kin
from test_abi_cpu import declared_functions
from test_krylov_cpu import hier


def test_header_declares_the_multi_rhs_entry_points():
    assert {"amgd_krylov_device_n", "amgd_krylov_n_stats", "amgd_crs_krylov_n"} <= declared_functions()


@pytest.mark.parametrize("case", kin.CASES)
def test_columns_end_after_different_iteration_counts(case):
    """with the guesses at restart 5: at least 5 distinct iteration counts, a 0 among them, every
    column converged within 20 iterations, some column restarted at least twice"""
    runs = kin.reference(case, hier(case), 5, True)
    its = [r["its"] for r in runs]
    print(case, its, [r["restarts"] for r in runs])
    assert all(r["rc"] == 0 for r in runs), [r["rc"] for r in runs]
    assert len(set(its)) >= 5, its
    assert 0 in its
    assert max(its) <= 20, its
    assert max(r["restarts"] for r in runs) >= 2
