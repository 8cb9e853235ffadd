"""The blocked Q-factor kernel (k_qfactor_blk, supports of 33..1024 points) against the
oracle's restatement of interp's Q loop, bit for bit: every tier edge and every residue of
the support size modulo the block of k-steps, with the kernel's switches (qf_chain: the
block's own rows in registers, read-ahead chains; qf_pass: grouped LDS reads in the two
passes) on and off, and with the grid capped so
that one block factors several supports in sequence (state carried from one support into
the next would show there and nowhere else)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import refops
import omp_amg_amd as oa

pytestmark = pytest.mark.gpu

M = 20
TIER_SIZES = {
    64: [33, 34, 35, 36, 47, 48, 49, 63, 64],
    128: [65, 127, 128],
    256: [129, 191, 192, 193, 255, 256],
    512: [257, 320, 511, 512],
    1024: [513, 769, 1021, 1022, 1023, 1024],
}
# >= 7 supports per tier, sizes spread over the tier (both ends, partial last blocks)
CARRY_SIZES = {
    64: [64, 33, 63, 40, 34, 49, 35, 58],
    128: [128, 65, 127, 80, 66, 101, 67],
    256: [256, 129, 255, 150, 130, 193, 131],
    512: [512, 257, 511, 300, 258, 385, 259],
    1024: [1024, 513, 1023, 600, 514, 769, 515],
}


@functools.lru_cache(maxsize=None)
def _matrix():
    from omp_amg_amd import problems
    Ai, Aj, Av = problems.poisson3d(M, 27)
    o = np.lexsort((Aj, Ai))
    aro, acol, aa = problems.coo_to_csr_np(np.asarray(Ai)[o], np.asarray(Aj)[o], np.asarray(Av)[o])
    return refops.Csr(M ** 3, M ** 3, aro, acol, aa)


def _supports(sizes, seed):
    """a sorted random subset of a contiguous index window of 3 nz per support"""
    rng = np.random.default_rng(seed)
    out = []
    for nz in sizes:
        if nz == 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        lo = int(rng.integers(0, M ** 3 - 3 * nz))
        out.append(np.sort(rng.choice(np.arange(lo, lo + 3 * nz), size=nz, replace=False)))
    return out


def _w_of(supports):
    ro = np.concatenate(([0], np.cumsum([len(s) for s in supports])))
    cols = np.concatenate(supports).astype(np.int64)
    return refops.Csr(len(supports), M ** 3, ro, cols, np.ones(len(cols)))


def _oracle_qfactor(W, A):
    lib = C.CDLL(os.path.join(os.path.dirname(__file__), "..", "oracle", "build", "liboracle.so"))
    nzs = np.diff(W.row_off)
    Q = np.zeros(int((nzs * (nzs + 1) // 2).sum()) + 1)
    wro = np.ascontiguousarray(W.row_off, dtype=np.uint64)
    wcol = np.ascontiguousarray(W.col, dtype=np.uint32)
    aro = np.ascontiguousarray(A.row_off, dtype=np.uint64)
    acol = np.ascontiguousarray(A.col, dtype=np.uint32)
    aa = np.ascontiguousarray(A.a, dtype=np.float64)
    lib.oracle_qfactor(C.c_uint32(W.rn), wro.ctypes.data_as(C.c_void_p), wcol.ctypes.data_as(C.c_void_p),
                       C.c_uint32(A.rn), aro.ctypes.data_as(C.c_void_p), acol.ctypes.data_as(C.c_void_p),
                       aa.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p))
    return Q[:-1]


def _split(Q, supports):
    """the packed factor of each support, out of the oracle's concatenation"""
    tn = [len(s) * (len(s) + 1) // 2 for s in supports]
    off = np.concatenate(([0], np.cumsum(tn)))
    out = [Q[off[q]:off[q + 1]] for q in range(len(supports))]
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _sizes_case():
    """one support of every listed size, an empty and a 1-point support, and the oracle's
    factors (computed once, read-only)"""
    sizes = [n for t in sorted(TIER_SIZES) for n in TIER_SIZES[t]] + [0, 1]
    sup = _supports(sizes, 151)
    W = _w_of(sup)
    ref = _oracle_qfactor(W, _matrix())
    ref.flags.writeable = False
    return W, ref


@functools.lru_cache(maxsize=None)
def _carry_case(tier):
    sup = _supports(CARRY_SIZES[tier], 152 + tier)
    return sup, _split(_oracle_qfactor(_w_of(sup), _matrix()), sup)


def _factor(W, chain, pas, grid=0):
    oa.qf_split(0)
    oa.qf_chain(chain)
    oa.qf_pass(pas)
    oa.qf_grid(grid)
    try:
        return oa.test_csr_op(5, W, _matrix())
    finally:
        oa.qf_grid(0)
        oa.qf_pass(-1)
        oa.qf_chain(-1)
        oa.qf_split(-1)


# every switch on, each part alone off, all off, and the defaults (-1); qf_pass acts on
# the 512 and 1024 tiers only, so on the smaller tiers its two settings run the same kernel
SWITCHES = [(1, 1), (0, 1), (1, 0), (0, 0), (-1, -1)]


@pytest.mark.parametrize("chain,pas", SWITCHES)
def test_qfactor_blk_sizes_bitexact(chain, pas):
    W, ref = _sizes_case()
    oa.route_stats(reset=True)
    X = _factor(W, chain, pas)
    r = oa.route_stats(reset=True)
    assert r["qf_t512"] > 0 and r["qf_t1024"] > 0, r
    assert X.nnz == len(ref)
    got = np.ascontiguousarray(X.a[:len(ref)]).view(np.uint64)
    bad = np.flatnonzero(got != ref.view(np.uint64))
    assert bad.size == 0, (chain, pas, bad[:8], bad.size)


@pytest.mark.parametrize("order", ["mixed", "descending", "ascending"])
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("tier", sorted(CARRY_SIZES))
def test_qfactor_blk_carried_state(tier, grid, order):
    """7 or 8 supports of one tier on 1 or 3 blocks: every block factors two or more in
    sequence, larger after smaller and smaller after larger"""
    sup, refs = _carry_case(tier)
    n = len(sup)
    perm = list(range(n))
    if order == "descending":
        perm.sort(key=lambda q: -len(sup[q]))
    elif order == "ascending":
        perm.sort(key=lambda q: len(sup[q]))
    W = _w_of([sup[q] for q in perm])
    ref = np.concatenate([refs[q] for q in perm])
    for chain, pas in SWITCHES[:4]:
        X = _factor(W, chain, pas, grid)
        assert X.nnz == len(ref)
        got = np.ascontiguousarray(X.a[:len(ref)]).view(np.uint64)
        bad = np.flatnonzero(got != ref.view(np.uint64))
        assert bad.size == 0, (tier, grid, order, chain, pas, bad[:8], bad.size)
