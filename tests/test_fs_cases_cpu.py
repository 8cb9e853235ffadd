"""The inputs of the find_support tests (tests/fs_cases.py) and their host references, checked
without a GPU: every case keeps the property it exists for, the numpy restatement of one
selection sweep picks the first of every repeated maximum the builders planted, and the
restatement of the whole loop (refops.find_support) equals the oracle's own find_support
(oracle/amg_oracle.c, exported) on every loop case, sweep count included."""
import numpy as np
import pytest

import fs_cases as fc
import refops


def _col(case, c):
    T = refops.Csc(case.R)
    return T.row[T.ro[c]:T.ro[c + 1]]


@pytest.mark.parametrize("case", fc.sel_cases(), ids=lambda c: c.name)
def test_selection_case(case):
    """one pair per bad column; the first planted maximum wins; nothing else changes"""
    ref = refops.fs_select(case.R, case.rs, case.w, case.sumR, case.thr)
    assert ref["removed"] and np.array_equal(ref["sel"][:, 1], case.bad)
    chosen = dict(zip(ref["sel"][:, 1].tolist(), ref["sel"][:, 0].tolist()))
    for c, pos in case.ties.items():
        assert len(pos) >= 1 and chosen[c] == _col(case, c)[pos[0]], (c, pos)
    changed = np.nonzero(ref["Ra"].view(np.uint64) != np.asarray(case.R.a).view(np.uint64))[0]
    assert len(changed) <= len(case.bad)                  # -0 / +0 maxima may keep their bits
    assert (ref["Ra"][changed] == 0.0).all() and not np.signbit(ref["Ra"][changed]).any()
    untouched = np.setdiff1d(np.arange(case.nc), case.bad)
    assert np.array_equal(ref["sumR"][untouched], case.sumR[untouched])
    if hasattr(case, "expect_dup_row"):
        assert (ref["sel"][:, 0] == case.expect_dup_row).sum() >= 2     # one row, two bad columns
    # above every w: no bad column, nothing changes
    none = refops.fs_select(case.R, case.rs, case.w, case.sumR, 10.0)
    assert len(none["sel"]) == 0 and not none["removed"] and np.array_equal(none["Ra"], case.R.a)


@pytest.mark.parametrize("case", fc.sel_cases(), ids=lambda c: c.name)
def test_selection_windows(case):
    """the windowed form selects the bad columns of its window, globally numbered, and leaves
    R, rs and sumR alone; one window holds no bad column, one a single bad column"""
    whole = refops.fs_select(case.R, case.rs, case.w, case.sumR, case.thr)
    counts = []
    for c0, c1 in case.windows:
        ref = refops.fs_select(case.R, case.rs, case.w, case.sumR, case.thr, c0, c1, windowed=True)
        inside = (whole["sel"][:, 1] >= c0) & (whole["sel"][:, 1] < c1)
        assert np.array_equal(ref["sel"], whole["sel"][inside])
        assert np.array_equal(ref["Ra"], case.R.a) and np.array_equal(ref["rs"], case.rs)
        counts.append(len(ref["sel"]))
    if case.name.startswith("G"):
        assert counts[2] == 0 and counts[3] == 1 and 0 < counts[1] < counts[0]


def test_long_case_chunks():
    """the planted maxima of the long columns lie where the chunked kernels can go wrong"""
    case = fc.case_long()
    ch = fc.FSL_CH
    t = {n: case.ties[case.where[n]] for n in fc.LONG_LENS}
    assert t[2048][0] == ch - 1 and t[2049][0] == ch                 # last of chunk 0 / first of chunk 1
    assert t[4097] == (ch - 1, ch, 2 * ch)                            # three chunks, the first wins
    assert t[6000][0] // ch == 0 and t[6000][1] // ch == 2            # equal in chunks 0 and 2
    assert {p % 256 for p in t[2047]} == {3} and t[2047][1] - t[2047][0] == 256   # one thread, two strides
    assert (t[4096][1] - t[4096][0]) == 64                            # two wavefronts of one block
    for n in fc.LONG_LENS:
        assert -(-n // ch) == {2047: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3, 6000: 3}[n]


def test_expand_cases():
    for name, M, rows, longs in fc.expand_cases():
        out, st = refops.fs_expand(M, rows, np.zeros(M.cn, dtype=np.uint32), 5)
        assert len(out) > 8 and len(np.unique(rows)) < len(rows)       # duplicates in the list
        again, st2 = refops.fs_expand(M, rows, st, 5)
        assert len(again) == 0 and np.array_equal(st, st2)
        assert (name == "thread") == (len(M.a) < 16 * M.rn)


def test_reduction_vectors():
    for n in fc.RED_N:
        for name, a in fc.red_vectors(n):
            assert len(a) == n and (a >= 0).all()
            i = int(np.argmax(a))
            if name in ("max_last", "two_blocks", "repeated", "strides"):
                assert a[i] == 2.0
            if name == "max_last":
                assert i == n - 1
            if name == "repeated":
                assert i == 130 and (a == 2.0).sum() >= 3
            if name == "two_blocks":
                assert i == n - 259 and i // 256 != (n - 1) // 256
            if name == "strides":
                assert i == 256 and a[fc.RED_FULL] == 2.0


def _run_loop(R, goal):
    Sk, tr = refops.find_support(R, goal)          # raises on every UB() exit of the library
    return Sk, tr


def test_loop_orphan(oracle_lib):
    """ends by max(v) < goal with no UB exit, within 400 sweeps, at least 100 selections from a
    column of more than 2 * FSL_CH entries; the host loop equals the oracle's"""
    R, goal = fc.loop_orphan()
    Sk, tr = _run_loop(R, goal)
    assert tr["sweeps"] <= 400
    long_cols = np.nonzero(tr["col_len"] > 2 * fc.FSL_CH)[0]
    nlong = sum(int(np.isin(s[:, 1], long_cols).sum()) for s in tr["sels"])
    assert nlong >= 100 and len(tr["sels"]) == tr["sweeps"] - 1
    assert fc.default_long(len(R.a), R.cn) == 4096 and tr["col_len"][0] == 5000
    So, sweeps, ub = fc.oracle_find_support(oracle_lib, R, goal)
    assert ub == 0 and sweeps == tr["sweeps"] and refops.same(Sk, So)


def test_loop_banded(oracle_lib):
    """10-100 sweeps, at least half of them on the incremental path, at least one cap
    overflow (a sweep after few selections that still takes full products)"""
    R, goal = fc.loop_banded()
    Sk, tr = _run_loop(R, goal)
    n_inc = sum(tr["inc_next"])
    assert 10 <= tr["sweeps"] <= 100 and 2 * n_inc >= tr["sweeps"]
    cap_c = R.cn // 4 + 1
    assert any(not ok and len(s) <= cap_c for ok, s in zip(tr["inc_next"], tr["sels"]))
    assert min(len(s) for s in tr["sels"]) >= 5 and len(R.a) >= 32 * R.cn
    So, sweeps, ub = fc.oracle_find_support(oracle_lib, R, goal)
    assert ub == 0 and sweeps == tr["sweeps"] and refops.same(Sk, So)


def test_loop_tiny(oracle_lib):
    R = fc.loop_tiny()
    first = refops.fs_products(R, refops.Csc(R), np.asarray(R.a))
    mv = float((first[3] / first[1]).max())
    Sk, tr = _run_loop(R, 1.01 * mv)                # above the first max(v): no selection
    assert tr["sweeps"] == 1 and len(Sk.col) == 0
    So, sweeps, ub = fc.oracle_find_support(oracle_lib, R, 1.01 * mv)
    assert ub == 0 and sweeps == 1 and refops.same(Sk, So)
    Sk, tr = _run_loop(R, 0.9 * mv)
    So, sweeps, ub = fc.oracle_find_support(oracle_lib, R, 0.9 * mv)
    assert tr["sweeps"] == 2 and len(Sk.col) == 2 and ub == 0 and sweeps == 2 and refops.same(Sk, So)


def test_loop_ub_exits_raise():
    """the restatement refuses the undefined paths instead of returning something"""
    R = fc.loop_tiny()
    one = type(R)(1, 3, np.array([0, 3]), np.array([0, 1, 2]), np.array([0.5, 0.25, 1.0]))
    with pytest.raises(refops.FsUndefined):
        refops.find_support(one, 0.1)               # nf <= 1
    with pytest.raises(refops.FsUndefined):
        refops.find_support(R, 0.0)                 # the goal cannot be met: nothing left to remove
