"""Flexible GMRES on the row-partitioned hierarchy, on the host (DESIGN.md "Krylov on the
row-partitioned hierarchy"), without a GPU: the fused path's dot -- every rank's own sum, the
ranks' sums added in rank order -- keeps the solve converging in the sequential count on the
committed fixtures, the documented collective count is what the loop makes, and the public
header declares the new entry point."""
import numpy as np
import pytest

import refkrylov
import refsolve
from test_abi_cpu import declared_functions
from test_krylov_cpu import CASES, RTOL, hier, solve


def rank_order_dot(split):
    """a . b as the fused partitioned path forms it, in the restatement's terms: per rank the
    left-to-right sum of the rounded products of its rows (a rank without rows: +0), then
    s = p_0; s = s + p_1; ..."""
    def dot(a, b):
        p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        parts = [refsolve.seq_sum(p[split[r]:split[r + 1]]) for r in range(len(split) - 1)]
        s = parts[0]
        for q in parts[1:]:
            s = s + q
        return s
    return dot


def cut(kind, n, N, seed):
    if kind == "even":
        return [n * p // N for p in range(N + 1)]
    rng = np.random.default_rng(seed)
    while True:                                        # ragged: unequal, possibly empty ranges
        s = [0] + sorted(rng.integers(0, n + 1, N - 1).tolist()) + [n]
        if len(set(np.diff(s).tolist())) > 1:
            return s


# every rank count and both cuts, spread over the fixtures and the two restart lengths (a run of
# the restatement takes a second or so: one per fixture and restart)
PLAN = [(case, restart, (2, 3, 4, 8)[(i + j) % 4], ("even", "ragged")[(i + j // 2) % 2])
        for i, case in enumerate(CASES) for j, restart in enumerate((30, 5))]


@pytest.mark.parametrize("case,restart,N,kind", PLAN)
def test_rank_order_dots_converge_in_the_sequential_count(case, restart, N, kind):
    """rc 0 in exactly the count of the sequential restatement, the recomputed residual under
    rtol ||b||: the fused criteria of the GPU tests (its within one, residual within
    rtol (1 + 1e-3) ||b||) leave room"""
    h = hier(case)
    b, seq = solve(case, restart)
    n = int(h.levels[0].n)
    res = refkrylov.fgmres(h, b, rtol=RTOL, restart=restart, maxit=20, dot=rank_order_dot(cut(kind, n, N, N)))
    assert res["rc"] == 0 and res["its"] == seq["its"] and res["restarts"] == seq["restarts"], (res["its"], seq["its"])
    rel = np.linalg.norm(b - refsolve.csr_matvec(h.levels[0].A, res["x"])) / np.linalg.norm(b)
    print(case, restart, N, kind, "its", res["its"], "relative residual", rel)
    assert rel <= RTOL, rel


def test_one_rank_dot_is_the_sequential_dot():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(1001), rng.standard_normal(1001)
    assert rank_order_dot([0, 1001])(a, b) == refkrylov.seq_dot(a, b)
    assert rank_order_dot([0, 0, 1001, 1001])(a, b) == refkrylov.seq_dot(a, b)     # ranks without rows add +0


def count_formula(its, restarts, cyc, px, guess, complete):
    return 1 + guess * (px + 1) + its * (cyc + px + 3) + (restarts + 1) * (px + 1) + (1 if complete else 0)


def count_loop(inner, cyc, px, guess, complete):
    """the collectives of a fused call, walked as amgd_krylov.c's loop makes them; inner: the
    inner iterations of every restart"""
    c = 1                                   # ||b||^2: one combine
    if guess:
        c += px + 1                         # r = b - A x0: the product's exchange, ||r||^2
    for k in inner:
        for _ in range(k):
            c += cyc                        # z_j = cycle(v_j)
            c += px                         # w = A z_j
            c += 3                          # pass 1, pass 2, ||w||^2
        c += px + 1                         # the true residual and its norm
    return c + (1 if complete else 0)


@pytest.mark.parametrize("inner", [[1], [7], [5, 5, 3], [30, 30, 1]])
@pytest.mark.parametrize("cyc,px", [(0, 0), (1, 0), (1, 1), (9, 1), (14, 1)])
def test_count_formula_is_the_loops(inner, cyc, px):
    for guess in (0, 1):
        for complete in (False, True):
            assert count_loop(inner, cyc, px, guess, complete) == \
                count_formula(sum(inner), len(inner) - 1, cyc, px, guess, complete)


def test_header_declares_the_comm_stats():
    assert "amgd_krylov_comm_stats" in declared_functions()
