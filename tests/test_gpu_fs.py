"""find_support's kernels and its sweep loop against host references, bit for bit
(tests/fs_cases.py builds the inputs, tests/refops.py restates the reference operations,
tests/test_fs_cases_cpu.py checks both without a GPU).

  selection   amgd_fs_select, amgd_spmv_amax + amgd_fs_select_amx, and the windowed
              amgd_fs_select_ex(perm NULL, resum 0) of the partitioned driver: every
              k_fs_select<G> instance at the G*8 unroll edge, repeated maxima across lanes,
              unroll slots, wavefronts and chunks, signed zeros, the grid-wide long-column
              kernels with multi-chunk columns and more than 256 long columns
  expansion   amgd_fs_expand (thread, wave and long-row kernels) and amgd_fs_claim_ext
  reductions  amgd_max_first / max_first2 / count_gt at the block-geometry edges,
              amgd_vdiv_guard, and the small matrix kernels around the loop
  whole loop  find_support itself in every mode, skeleton and sweep count

The amx variant runs on the cases whose mean column length reaches the lane SpMV kernels
(nnz >= 32 nc): only there does amgd_spmv_amax deliver the maxima, in the tests as in
find_support.  On them a return of 0 fails the test.
The device's nremoved is a flag (0 / 1), compared as such."""
import functools

import numpy as np
import pytest

import omp_amg_amd as oa

import fs_cases as fc
import refops

pytestmark = pytest.mark.gpu

SEL = {c.name: c for c in fc.sel_cases()}
AMX = [n for n, c in SEL.items() if c.amx]
WINDOWS = [(n, k) for n, c in SEL.items() for k in range(len(c.windows))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _defaults():
    yield
    oa.fs_long(-1)
    oa.fs_amx(-1)
    oa.spmv_sl_min(-1)
    oa.spmv_tab(-1)


@functools.lru_cache(maxsize=None)
def _ref(name, thr=None, win=None):
    c = SEL[name]
    c0, c1 = (0, None) if win is None else c.windows[win]
    return refops.fs_select(c.R, c.rs, c.w, c.sumR, c.thr if thr is None else thr, c0, c1,
                            windowed=win is not None)


def _same_selection(got, ref):
    order = np.argsort(got["sel"][:, 1], kind="stable")
    assert got["nsel"] == len(ref["sel"])                      # one pair per bad column
    assert np.array_equal(got["sel"][order], ref["sel"])
    assert (got["nremoved"] != 0) == ref["removed"]
    for k in ("Ra", "Rta", "rs", "sumR"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("fs_long", [-1, 8], ids=["long_default", "long8"])
@pytest.mark.parametrize("pin", [1, 0], ids=["pinned", "unpinned"])
@pytest.mark.parametrize("name", list(SEL))
def test_select_plain(name, pin, fs_long):
    """amgd_fs_select.  Unpinned, amgd_max_row_len is UINT32_MAX: the long-column kernels
    run on whatever is longer than fs_long(), an empty list for the G cases by default."""
    c = SEL[name]
    oa.fs_long(fs_long)
    got = oa.test_fs_select("plain", c.R, c.rs, c.w, c.sumR, c.thr, pin=bool(pin))
    _same_selection(got, _ref(name))


@pytest.mark.parametrize("tab", [-1, 1], ids=["tab_default", "tab_on"])
@pytest.mark.parametrize("pin", [1, 0], ids=["pinned", "unpinned"])
@pytest.mark.parametrize("name", AMX)
def test_select_amx(name, pin, tab):
    """amgd_spmv_amax(R', rs) then amgd_fs_select_amx: the fused first maxima (the paired
    lane kernel, or the gather-table kernel on a pinned R' with tables on) select what the
    selection's own pass selects"""
    c = SEL[name]
    oa.spmv_sl_min(0)
    oa.spmv_tab(tab)
    got = oa.test_fs_select("amx", c.R, c.rs, c.w, c.sumR, c.thr, pin=bool(pin))
    assert got["amax"] == 1, "amgd_spmv_amax delivered no maxima"
    _same_selection(got, _ref(name))


@pytest.mark.parametrize("fs_long", [-1, 8], ids=["long_default", "long8"])
@pytest.mark.parametrize("pin", [1, 0], ids=["pinned", "unpinned"])
@pytest.mark.parametrize("name,win", WINDOWS, ids=[f"{n}-w{k}" for n, k in WINDOWS])
def test_select_windowed(name, win, pin, fs_long):
    """amgd_fs_select_ex on rows [c0, c1) of R' with perm NULL and resum 0: sel_j global, only
    the window's R' values zeroed, R's values, rs and sumR untouched"""
    c = SEL[name]
    c0, c1 = c.windows[win]
    oa.fs_long(fs_long)
    got = oa.test_fs_select("windowed", c.R, c.rs, c.w, c.sumR, c.thr, pin=bool(pin), c0=c0, c1=c1)
    ref = _ref(name, win=win)
    _same_selection(got, ref)
    assert np.array_equal(bits(got["Ra"]), bits(c.R.a)) and np.array_equal(bits(got["rs"]), bits(c.rs))
    assert np.array_equal(bits(got["sumR"]), bits(c.sumR))
    assert ((got["sel"][:, 1] >= c0) & (got["sel"][:, 1] < c1)).all()


@pytest.mark.parametrize("variant", ["plain", "amx", "windowed"])
@pytest.mark.parametrize("name", ["G4", "G32", "long"])
def test_select_no_bad_column(name, variant):
    """thr above every w: nothing changes and nremoved is 0"""
    c = SEL[name]
    if variant == "amx" and not c.amx:
        variant = "plain"
    oa.spmv_sl_min(0)
    c0, c1 = c.windows[1] if variant == "windowed" else (0, None)
    got = oa.test_fs_select(variant, c.R, c.rs, c.w, c.sumR, 10.0, c0=c0, c1=c1)
    assert got["nsel"] == 0 and got["nremoved"] == 0
    _same_selection(got, _ref(name, thr=10.0))


# ------------------------------------------------------------------------------ expansion
EXP = {name: (M, rows, longs) for name, M, rows, longs in fc.expand_cases()}
EXP_IDS = [(n, l, p) for n, (_, _, longs) in EXP.items() for l in longs for p in (1, 0)]


def _prestamp(M, rows, tag, seed):
    """stamps before the call: a third of the listed rows' neighbours already claimed (tag),
    the rest holding older tags"""
    rng = np.random.default_rng(seed)
    st = rng.choice(np.array([0, tag - 1, tag + 1, 0xfffffff0], dtype=np.uint32), size=M.cn)
    nb, _ = refops.fs_expand(M, rows, st, tag)
    st[nb[rng.random(len(nb)) < 0.33]] = tag
    return st


@pytest.mark.parametrize("name,fs_long,pin", EXP_IDS, ids=[f"{n}-long{l}-pin{p}" for n, l, p in EXP_IDS])
def test_expand(name, fs_long, pin):
    """the distinct unclaimed neighbours, whatever the order; past cap only the count; the
    claimed stamps become tag, every other stamp stays; a repeat with the same tag finds none"""
    M, rows, _ = EXP[name]
    tag = 7
    st0 = _prestamp(M, rows, tag, 1)
    want, st_want = refops.fs_expand(M, rows, st0, tag)
    n = len(want)
    assert 0 < n < len(refops.fs_expand(M, rows, np.zeros(M.cn, dtype=np.uint32), tag)[0])
    oa.fs_long(fs_long)
    for cap in (n + 5, n, n - 1, 0):
        cnt, out, st, guard = oa.test_fs_expand(M, rows, st0, tag, cap, pin=bool(pin))
        assert cnt == n and guard == 0xffffffff, (cap, cnt, n)
        assert np.array_equal(st, st_want)
        if cap >= n:
            assert np.array_equal(np.sort(out), want)
        else:
            assert len(out) == cap and len(np.unique(out)) == cap and np.isin(out, want).all()
        cnt2, out2, st2, _ = oa.test_fs_expand(M, rows, st, tag, max(cap, 1), pin=bool(pin))
        assert cnt2 == 0 and len(out2) == 0 and np.array_equal(st2, st_want)


def test_claim_ext():
    """amgd_fs_claim_ext behind `have` entries already in the list; ids twice in the call and
    ids already claimed are not appended again"""
    rng = np.random.default_rng(2)
    ns, tag = 4000, 9
    have = rng.choice(ns, 37, replace=False).astype(np.uint32)
    st0 = rng.choice(np.array([0, tag - 1, tag + 5], dtype=np.uint32), size=ns)
    st0[have] = tag
    ids = np.concatenate([rng.choice(ns, 900, replace=False), have[:10], rng.choice(ns, 300)]).astype(np.uint32)
    fresh = np.unique(ids[st0[ids] != tag]).astype(np.int64)
    n = len(have) + len(fresh)
    st_want = st0.copy()
    st_want[fresh] = tag
    assert len(fresh) < len(np.unique(ids)) < len(ids)
    for cap in (n + 3, n, n - 1, len(have), 0):
        cnt, out, st, guard = oa.test_fs_claim_ext(ids, st0, tag, have[:min(len(have), cap)], cap)
        hv = min(len(have), cap)
        want_cnt = hv + len(fresh)
        assert cnt == want_cnt and guard == 0xffffffff and np.array_equal(st, st_want)
        assert np.array_equal(out[:hv], have[:hv])
        if cap >= want_cnt:
            assert np.array_equal(np.sort(out[hv:]), fresh)
        else:
            assert len(np.unique(out[hv:])) == cap - hv and np.isin(out[hv:], fresh).all()
    cnt, out, st, _ = oa.test_fs_claim_ext(np.zeros(0, dtype=np.uint32), st0, tag, have, 64)
    assert cnt == len(have) and np.array_equal(st, st0)


# ----------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("n", fc.RED_N)
def test_reductions(n):
    """extr_op (amg_setup.c:3281: from a[0], strict >: the first maximum), the count and
    maximum of amg_setup.c:761-768 (strict >, the maximum from 0) and v = w2 ./ w with
    v(w == 0) = 0 (:1306-1311), at lengths around the reduction's block geometry
    (256 threads, at most 1024 blocks).  The device starts its maximum at -DBL_MAX where
    the reference starts at a[0]: they differ only for -inf or NaN input, which the
    setup cannot produce (R >= 0, divisions by zero are guarded)."""
    rng = np.random.default_rng(n + 1)
    for name, a in fc.red_vectors(n) + [("negative", -1.0 - fc.red_vectors(n)[0][1])]:
        i = int(np.argmax(a))
        assert oa.test_fs_vec("max_first", a) == (float(a[i]), i), name
        b = a[::-1].copy()
        v, vi, mb = oa.test_fs_vec("max_first2", a, b)
        assert (v, vi, mb) == (float(a[i]), i, float(b.max())), name
        for thr in (float(a[i]), float(np.sort(a)[n // 2]), -5.0):
            cnt, mx = oa.test_fs_vec("count_gt", a, thr=thr)       # values equal to thr do not count
            assert (cnt, mx) == (int((a > thr).sum()), max(float(a.max()), 0.0)), (name, thr)
    num = rng.standard_normal(n)
    den = rng.choice(np.array([0.0, -0.0, 1.0, 3.0, -0.7, 1e-300]), size=n)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(den == 0.0, 0.0, num / den)
    assert np.array_equal(bits(oa.test_fs_vec("vdiv_guard", num, den)), bits(want))


def test_small_matrix_kernels():
    """csc_gemv with and without x, list_rowsum in both branches, bad_rows, skel_binarize in
    both modes, scale_diag_match (amg_setup.c:821-837)"""
    rng = np.random.default_rng(5)
    M = EXP["orphan"][0]
    A = type(M)(M.rn, M.cn, M.row_off, M.col, rng.standard_normal(len(M.col)))
    T = refops.Csc(A)
    x = rng.standard_normal(A.rn)
    assert np.array_equal(bits(oa.test_fs_mat("csc_gemv", A, x=x)),
                          bits(refops.ordered_rowsum(T.ro, A.a[T.perm] * x[T.row])))
    assert np.array_equal(bits(oa.test_fs_mat("csc_gemv", A)), bits(refops.ordered_rowsum(T.ro, A.a[T.perm])))
    rows = np.concatenate([rng.choice(A.rn, 40, replace=False), [int(np.argmax(np.diff(A.row_off)))]])
    z0 = rng.standard_normal(A.rn)
    want = z0.copy()
    want[rows] = refops.ordered_rowsum(A.row_off, A.a)[rows]
    for long_rows in (0, 1):
        assert np.array_equal(bits(oa.test_fs_mat("list_rowsum", A, rows=rows, iarg=long_rows, z0=z0)), bits(want))
    vals = rng.choice(np.array([2.0, 1.0, 0.5, 0.0, -0.0, -2.0]), size=len(M.col), p=[.02, .5, .2, .1, .08, .1])
    S = type(M)(M.rn, M.cn, M.row_off, M.col, vals)
    mask, cnt = oa.test_fs_mat("bad_rows", S)
    want_mask = np.array([(vals[M.row_off[i]:M.row_off[i + 1]] == 2.0).any() for i in range(M.rn)])
    assert np.array_equal(mask != 0, want_mask) and cnt == want_mask.sum() and 0 < cnt < M.rn
    assert np.array_equal(bits(oa.test_fs_mat("skel_binarize", S, iarg=0)), bits(np.where(vals == 2.0, 1.0, vals)))
    assert np.array_equal(bits(oa.test_fs_mat("skel_binarize", S, iarg=1)), bits(np.where(vals != 0.0, 1.0, vals)))
    W = refops.rand_csr(rng, 300, 300, 0.05)
    for i in range(0, 300, 3):                         # diagonal entries on a third of the rows
        k = W.row_off[i]
        if W.row_off[i + 1] > k:
            W.col[k:W.row_off[i + 1]] = np.sort(np.concatenate([[i], np.setdiff1d(W.col[k:W.row_off[i + 1]], [i])])
                                                )[:W.row_off[i + 1] - k]
    v = rng.standard_normal(300)
    wuc = rng.choice(np.array([0.0, -0.0, 0.5, 3.0, -1.7]), size=300)
    want = np.array(W.a)
    ndiag = 0
    for i in range(300):
        for k in range(W.row_off[i], W.row_off[i + 1]):
            if wuc[i] != 0.0 and W.col[k] == i:
                want[k] = (v[i] / wuc[i]) * want[k]
                ndiag += 1
    assert ndiag > 20
    assert np.array_equal(bits(oa.test_fs_mat("scale_diag_match", W, x=v, y=wuc)), bits(want))


# ------------------------------------------------------------------------------ whole loop
@functools.lru_cache(maxsize=None)
def _loop(name):
    R, goal = {"orphan": fc.loop_orphan, "banded": fc.loop_banded}[name]()
    Sk, tr = refops.find_support(R, goal)
    return R, goal, Sk, tr


MODES = [(inc, amx, lg, first) for inc in ("0", "2") for amx in (0, 1) for lg in (-1, 8) for first in (0, 1)]


@pytest.mark.parametrize("inc,amx,fs_long,first", MODES,
                         ids=[f"inc{i}-amx{a}-long{l}-first{f}" for i, a, l, f in MODES])
@pytest.mark.parametrize("name", ["orphan", "banded"])
def test_find_support_loop(name, inc, amx, fs_long, first, monkeypatch, oracle_lib):
    """the loop itself: the skeleton and the sweep count of the host loop (orphan: every sum
    exact; banded: general values, the oracle's own find_support as the reference), in every
    mode; the incremental path serves exactly the sweeps whose three expansions stay within
    the caps, the fused maxima every other selecting sweep of a matrix that reaches the lane
    kernels.  orphan: 280-odd sweeps, each removing one entry of the 5 000-entry column (three
    chunks of the grid-wide selection at either threshold); every expansion overflows nf/4+1."""
    R, goal, Sk, tr = _loop(name)
    if name == "banded":
        So, sweeps, ub = fc.oracle_find_support(oracle_lib, R, goal)
        assert ub == 0 and sweeps == tr["sweeps"] and refops.same(So, Sk)
    oa.knob("fs_inc", int(inc))
    oa.fs_amx(amx)
    oa.fs_long(fs_long)
    oa.spmv_sl_min(0)
    oa.route_stats(reset=True)
    try:
        got, sweeps, ub = oa.test_find_support(R, goal, first=tr["first"] if first else None)
    finally:
        oa.knob("fs_inc", None)
    routes = oa.route_stats(reset=True)
    assert ub == 0 and sweeps == tr["sweeps"] == routes["fs_sweep"]
    assert refops.same(got, Sk)
    nsel = tr["sweeps"] - 1                                   # every sweep but the last selects
    by_inc = [inc == "2" and s > 1 and tr["inc_next"][s - 2] for s in range(1, tr["sweeps"] + 1)]
    assert routes["fs_inc"] == sum(by_inc)
    if name == "banded" and inc == "2":
        assert routes["fs_inc"] >= tr["sweeps"] // 2
    full_sel = [s for s in range(1, nsel + 1) if not by_inc[s - 1] and not (s == 1 and first)]
    delivers = amx == 1 and len(R.a) >= 32 * R.cn
    assert routes["fs_amx"] == (len(full_sel) if delivers else 0)
    if name == "banded" and amx == 1:
        assert routes["fs_amx"] > 0


def test_find_support_tiny(oracle_lib):
    """nf = 2; a goal above the first max(v): one sweep that selects nothing, an empty Sk"""
    R = fc.loop_tiny()
    f = refops.fs_products(R, refops.Csc(R), np.asarray(R.a))
    mv = float((f[3] / f[1]).max())
    for goal, first in ((1.01 * mv, None), (1.01 * mv, f), (0.9 * mv, None), (0.9 * mv, f)):
        Sk, tr = refops.find_support(R, goal)
        got, sweeps, ub = oa.test_find_support(R, goal, first=first)
        assert ub == 0 and sweeps == tr["sweeps"] and refops.same(got, Sk)
        assert refops.same(fc.oracle_find_support(oracle_lib, R, goal)[0], got)
    assert len(oa.test_find_support(R, 1.01 * mv)[0].col) == 0
