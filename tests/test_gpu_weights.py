"""The two consumers of the Q factors in solve_weights against the oracle, bit for bit, on the
cases of tests/weights_cases.py: the Q application (amgd_qapply: the lane-group, tiled, block
and grid-wide kernels of amgd_interp.hip) and the constraint operator interp_lmop (amgd_lmop:
QQ^t small / tiled, the three row-pull kernels, the QQ^t chunks, the dirty prefix, the general
walk with its row-skip tables, plain and pruned, and the redo after a missed column).  Every
test asserts by the route counters which kernel served it.  The oracle's results are computed
once per case (weights_cases caches them) and shared by the parametrisations."""
import numpy as np
import pytest

import omp_amg_amd as oa
import weights_cases as wc

pytestmark = pytest.mark.gpu


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ Q application
def _qapply(c, tile=-1, huge=-1, small=-1):
    oa.qa_tile(tile)
    oa.qa_huge(huge)
    oa.qa_small(small)
    oa.route_stats(reset=True)
    try:
        out = oa.test_qapply(c.Wt, c.A, c.Bt, c.u, c.lam)
    finally:
        oa.qa_tile(-1)
        oa.qa_huge(-1)
        oa.qa_small(-1)
    return out, oa.route_stats(reset=True)


@pytest.mark.parametrize("huge", [-1, 600], ids=["huge_default", "huge_600"])
@pytest.mark.parametrize("tile", [16, 32, 0], ids=["tile16", "tile32", "row_per_lane"])
def test_qapply_tiers(tile, huge):
    """one support per size around every kernel edge; at the lowered threshold the 1025- and
    1400-point supports take the grid-wide kernels and 513 / 600 the rewritten keep list"""
    c = wc.qa_tiers()
    out, r = _qapply(c, tile=tile, huge=huge)
    assert r["qa_s16"] > 0 and r["qa_s32"] > 0 and r["qa_mid"] > 0 and r["qa_blk"] > 0, r
    assert r["qa_huge"] == (2 if huge == 600 else 0), r
    _same(out, wc.oracle_interp(c))


def test_qapply_tiers_no_small_kernels():
    """every support of up to 512 points on the 33..512-point kernel"""
    c = wc.qa_tiers()
    out, r = _qapply(c, small=0)
    assert r["qa_s16"] == 0 and r["qa_s32"] == 0 and r["qa_mid"] > 0 and r["qa_blk"] > 0, r
    _same(out, wc.oracle_interp(c))


def test_qapply_many_small():
    """37 + 13 + 5 supports in mixed order: partly filled last blocks of both lane-group
    kernels, a rest after both split passes"""
    c = wc.qa_many_small()
    out, r = _qapply(c)
    assert r["qa_s16"] > 0 and r["qa_s32"] > 0 and r["qa_mid"] > 0 and r["qa_blk"] == 0, r
    _same(out, wc.oracle_interp(c))


# ------------------------------------------------------------------ interp_lmop
def _lmop(c, mode=0, small=-1, wave=-1, prune=-1):
    oa.lmop_mode(mode)
    oa.lmop_small(small)
    oa.lmop_wave(wave)
    oa.lmop_prune(prune)
    oa.lmop_qq_budget(c.budget)
    oa.lmop_stats(reset=True)
    oa.route_stats(reset=True)
    try:
        sa = oa.test_lmop(c.S, c.Wskel, c.A, c.u)
    finally:
        oa.lmop_mode(0)
        oa.lmop_small(-1)
        oa.lmop_wave(-1)
        oa.lmop_prune(-1)
        oa.lmop_qq_budget(-1)
    return sa, oa.lmop_stats(reset=True), oa.route_stats(reset=True)


@pytest.mark.parametrize("small", [1, 0], ids=["small_rows_thread", "small_rows_wave"])
def test_lmop_clean_bins(small):
    """S rows in every bin of the row pull, QQ^t by both kernels, one chunk"""
    c = wc.lmop_clean_bins()
    sa, st, r = _lmop(c, small=small)
    assert st["fast"] == 1 and st["general"] == 0 and st["misses"] == 0 and st["dirty_prefix"] == 0, st
    assert r["lmop_pull_wave"] > 0 and r["lmop_pull_blk"] > 0 and r["lmop_qq_tile"] > 0, r
    assert (r["lmop_pull_thr"] > 0) == bool(small) and r["lmop_chunks"] == 1, r
    _same(sa, wc.oracle_lmop(c)[0])


def test_lmop_clean_bins_general():
    """the general walk alone on the same operands"""
    c = wc.lmop_clean_bins()
    sa, st, r = _lmop(c, mode=1)
    assert st["fast"] == 0 and st["general"] == 1, st
    assert r["lmop_pull_thr"] + r["lmop_pull_wave"] + r["lmop_pull_blk"] + r["lmop_chunks"] == 0, r
    _same(sa, wc.oracle_lmop(c)[0])


def test_lmop_qq_chunks():
    """QQ^t under a 1 MB budget: S rows (one-thread and two-window ones among them) take their
    contributions from several chunks"""
    c = wc.lmop_qq_chunks()
    sa, st, r = _lmop(c)
    assert st["fast"] == 1 and st["general"] == 0 and st["misses"] == 0, st
    assert r["lmop_chunks"] == len(c.chunks()) >= 3, r
    _same(sa, wc.oracle_lmop(c)[0])


@pytest.mark.parametrize("prune", [0, 8], ids=["full", "pruned"])
@pytest.mark.parametrize("wave", [-1, 1, 0], ids=["wave64", "wave", "thread"])
def test_lmop_dirty_prefix(wave, prune):
    """column 0 walks first (off-row landings in the following row, over the 64-row maxima and
    over a whole 4096-row block), the clean columns are pulled on top"""
    c = wc.lmop_dirty_prefix()
    want, offrow, over = wc.oracle_lmop(c)
    assert offrow > 0 and over == 0
    sa, st, r = _lmop(c, wave=wave, prune=prune)
    assert st["dirty_prefix"] == 1 and st["fast"] == 1 and st["general"] == 0 and st["misses"] == 0, st
    assert (st["pruned"] > 0) == (prune == 8), st
    if prune == 0:                           # the unpruned walk: per wavefront unless turned off
        assert (r["lmop_wave"] > 0) == (wave != 0), r
    _same(sa, want)


def test_lmop_dirty_after_clean():
    """a dirty column above a clean one: everything on the general walk"""
    c = wc.lmop_dirty_after_clean()
    want, offrow, over = wc.oracle_lmop(c)
    assert offrow > 0 and over == 0
    sa, st, r = _lmop(c)
    assert st["general"] == 1 and st["fast"] == 0 and st["dirty_prefix"] == 0, st
    _same(sa, want)


@pytest.mark.parametrize("name", wc.HOLES)
def test_lmop_hole(name):
    """a stored entry of S is missing: whichever kernel pulls the row counts the miss -- also
    for a column before the first, between the two or behind the last window of a long row --
    and the exact walk redoes S, where the lost contribution lands on the next stored entry"""
    c = wc.lmop_hole(name)
    want, _, over = wc.oracle_lmop(c)
    assert over == 0
    sa, st, r = _lmop(c)
    assert st["misses"] > 0 and st["general"] == 1 and st["fast"] == 0, st
    _same(sa, want)
