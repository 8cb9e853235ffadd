"""Inputs of the find_support tests (tests/test_gpu_fs.py), built without a GPU and checked by
tests/test_fs_cases_cpu.py.  Every builder asserts the property its case exists for: which
k_fs_select<G> instance the matrix selects, the column lengths around the G*8 unroll edge,
where the repeated maxima lie, how many columns the long-column kernels get, which sweeps of
the whole loop the incremental path serves.

Selection cases are made of exact (dyadic) numbers: the wanted products p = R_ic * rs_i are
chosen first, rs_i is a power of two and R_ic = p / rs_i, so every tie is an exact tie and
every sum is exact.  w is synthetic (2 on the columns meant to be bad, 0.5 elsewhere, thr 1):
the selection reads it only to decide which columns are bad."""
import functools

import numpy as np

from omp_amg_amd.abi import Csr

import refops

FSL_CH = refops.FSL_CH
THR = 1.0
PMAX = 1.0                        # the enforced maximum product; ordinary ones are <= 40/64


def sel_G(nnz, nc):
    """lanes per column of k_fs_select (amgd_fs_select_ex)"""
    avg = (nnz + nc - 1) // nc
    G = 4
    while G < 64 and G * 2 <= avg:
        G <<= 1
    return G


def default_long(nnz, nc):
    """fs_long() of R' at the default setting"""
    return max(4096, 16 * (nnz // nc))


class SelCase:
    """R with rs, w, sumR, thr of one selection sweep; bad: the bad columns; ties: column ->
    the positions (within the column) holding the repeated maximum"""
    def __init__(self, name, nf, cols, rs, bad, w_special=None):
        self.name, self.nf, self.nc = name, nf, len(cols)
        ent = []
        for c, (rows, prods) in enumerate(cols):
            rows = np.asarray(rows, dtype=np.int64)
            assert len(rows) == len(prods) and (np.diff(rows) > 0).all() and (len(rows) == 0 or rows[-1] < nf)
            for i, p in zip(rows.tolist(), np.asarray(prods, dtype=np.float64).tolist()):
                ent.append((i, c, p / rs[i]))
        ent.sort(key=lambda t: (t[0], t[1]))
        ro = np.zeros(nf + 1, dtype=np.int64)
        for i, _, _ in ent:
            ro[i + 1] += 1
        self.R = Csr(nf, self.nc, np.cumsum(ro), np.array([t[1] for t in ent], dtype=np.int64),
                     np.array([t[2] for t in ent], dtype=np.float64))
        self.rs = np.asarray(rs, dtype=np.float64)
        T = refops.Csc(self.R)
        self.col_len = np.diff(T.ro)
        self.sumR = refops.ordered_rowsum(T.ro, self.R.a[T.perm])
        self.w = np.full(self.nc, 0.5)
        self.w[list(bad)] = 2.0
        for c, v in (w_special or {}).items():
            self.w[c] = v
        self.thr = THR
        self.bad = np.nonzero((self.w > THR) & (self.sumR != 0.0))[0]
        self.nnz = len(ent)
        self.G = sel_G(self.nnz, self.nc)
        self.amx = self.nnz >= 32 * self.nc          # amgd_spmv_amax delivers (lane kernels)
        self.windows = []


def _rows(rng, nf, n):
    return np.sort(rng.choice(nf, size=n, replace=False))


def _prods(rng, n):
    return rng.integers(1, 41, size=n) / 64.0


def _put_max(prods, pos):
    prods = np.array(prods)
    prods[list(pos)] = PMAX
    assert (np.delete(prods, list(pos)) < PMAX).all()
    return prods


@functools.lru_cache(maxsize=None)
def case_G(G):
    """mean column length selecting k_fs_select<G>; columns of 1, 8G-1, 8G, 8G+1 entries (and
    G-1, G, G+1, 2G+1), bad and adjacent in the list; the maximum repeated in different lanes,
    in different unroll slots of one lane, and past the first 8G entries; +0 / -0 / zeroed
    entries; an all-negative column; two bad columns with their maxima in one row; a column
    with w > thr and only zeros (sumR = 0: not bad); w == thr (not bad)."""
    rng = np.random.default_rng(100 + G)
    E = 8 * G
    nf = E + 60
    rs = 2.0 ** rng.integers(-1, 2, size=nf)
    fill = {4: 3, 8: 11, 16: 22, 32: 44, 64: 90}[G]
    cols, bad, ties = [], [], {}

    def add(n, tie=None, is_bad=True):
        p = _prods(rng, n)
        if tie:
            p = _put_max(p, tie)
            ties[len(cols)] = tuple(tie)
        if is_bad:
            bad.append(len(cols))
        cols.append((_rows(rng, nf, n), p))
        return len(cols) - 1

    # the unroll edge: one pass of the lanes covers 8G entries
    c_one = add(1)
    c_e1 = add(E - 1, tie=(E - 2 - G, E - 2))          # same lane, unroll slots 6 and 7
    c_e = add(E, tie=(G + 1, G + 2, E - 1))            # neighbouring lanes, and the last entry
    c_e2 = add(E + 1, tie=(E - 1, E))                  # last of the first pass, first of the second
    add(E + 1, tie=(E,))                               # the single entry of the second pass wins alone
    add(G - 1); add(G, tie=(0, G - 1)); add(G + 1, tie=(1, G)); add(2 * G + 1, tie=(G, 2 * G))
    add(2)
    # signed zeros and zeroed entries: the first of the equal maxima +0 / -0 wins
    n = G + 3
    p = -_prods(rng, n)
    p[[2, 3, n - 1]] = [-0.0, 0.0, 0.0]
    c_z = len(cols); bad.append(c_z); cols.append((_rows(rng, nf, n), p)); ties[c_z] = (2, 3, n - 1)
    p = _prods(rng, n)
    p[[0, 4]] = [0.0, -0.0]                           # zeroed entries below an ordinary maximum
    bad.append(len(cols)); cols.append((_rows(rng, nf, n), p))
    # all negative: > from -DBL_MAX still chooses one (the first of the two largest)
    p = -_prods(rng, n) - 1.0
    p[[1, G + 1]] = -0.5
    c_neg = len(cols); bad.append(c_neg); cols.append((_rows(rng, nf, n), p)); ties[c_neg] = (1, G + 1)
    # two bad columns whose maxima fall in one row
    r1, r2 = _rows(rng, nf, fill + 2), _rows(rng, nf, fill + 2)
    shared = int(r1[3])
    if shared not in r2:
        r2 = np.sort(np.concatenate([r2[r2 != r2[0]][:fill + 1], [shared]]))
    c_d1 = len(cols); bad.append(c_d1)
    cols.append((r1, _put_max(_prods(rng, len(r1)), [3])))
    c_d2 = len(cols); bad.append(c_d2)
    cols.append((r2, _put_max(_prods(rng, len(r2)), [int(np.nonzero(r2 == shared)[0][0])])))
    # only zeros under w > thr: sumR == 0, not bad, untouched
    c_zero = len(cols); bad.append(c_zero); cols.append((_rows(rng, nf, 3), np.array([0.0, -0.0, 0.0])))
    # fillers set the mean; every second one bad, a run of four clean ones, w == thr on one
    nfill = {4: 60, 8: 40, 16: 40, 32: 40, 64: 40}[G]
    f0 = len(cols)
    for k in range(nfill):
        add(fill + int(rng.integers(-1, 2)), is_bad=(k % 2 == 0 and not 8 <= k < 12))
    c_eq = f0 + 13
    case = SelCase(f"G{G}", nf, cols, rs, bad, w_special={c_eq: THR})
    case.ties = ties
    assert case.G == G, (case.G, G, case.nnz, case.nc)
    assert [case.col_len[c] for c in (c_one, c_e1, c_e, c_e2)] == [1, E - 1, E, E + 1]
    assert {c_one, c_e1, c_e, c_e2, c_z, c_neg, c_d1, c_d2} <= set(case.bad.tolist())
    assert c_zero not in case.bad and c_eq not in case.bad and case.sumR[c_zero] == 0.0
    assert (np.diff(case.bad) == 1).sum() >= 8          # bad columns adjacent in the list
    assert case.col_len.max() <= default_long(case.nnz, case.nc)   # no long column by default
    clean = [f0 + 8, f0 + 12]
    assert not set(range(*clean)) & set(case.bad.tolist())
    # windows of the windowed variant: all, from the middle, one without a bad column, one column
    mid = case.nc // 2
    case.windows = [(0, case.nc), (mid, case.nc), tuple(clean), (c_e2, c_e2 + 1)]
    case.expect_dup_row = shared
    return case


LONG_LENS = (2047, 2048, 2049, 4096, 4097, 6000)


@functools.lru_cache(maxsize=None)
def case_long():
    """columns of 2047 ... 6000 entries with the maximum at the chunk edges of the grid-wide
    selection (FSL_CH = 2048), 262 bad columns of 9-30 entries (long at fs_long(8): more than
    one 256-batch of k_fsl_prep's scan) and short bad columns between them.  At the default
    threshold (4096 here) exactly the 4097- and 6000-entry columns are long."""
    rng = np.random.default_rng(7)
    nf = 6100
    rs = 2.0 ** rng.integers(-1, 2, size=nf)
    ties = {2047: (3, 3 + 256),                 # one thread, successive strides
            2048: (2047,),                      # the last entry of chunk 0
            2049: (2048,),                      # the first (only) entry of chunk 1
            4096: (70, 70 + 64, 70 + 256, 2048 + 70),   # two wavefronts, two strides, two chunks
            4097: (2047, 2048, 4096),           # last of chunk 0, first of chunk 1, chunk 2's only entry
            6000: (100 + 64, 4096 + 5)}         # equal in chunks 0 and 2
    cols, bad, tie_of, where = [], [], {}, {}
    mids = [int(v) for v in rng.integers(9, 31, size=262)]
    shorts = [int(v) for v in rng.integers(1, 9, size=131)]
    plan = []
    for k, n in enumerate(mids):
        plan.append(n)
        if k % 2 == 0:
            plan.append(shorts[k // 2])
        if k % 44 == 20:
            plan.append(LONG_LENS[k // 44])
    assert sorted(n for n in plan if n > 30) == list(LONG_LENS)
    for n in plan:
        p = _prods(rng, n)
        c = len(cols)
        if n in ties:
            p = _put_max(p, ties[n]); tie_of[c] = ties[n]; where[n] = c
        elif n >= 12 and c % 3 == 0:
            t = (2, n - 1); p = _put_max(p, t); tie_of[c] = t
        if n > 8 or c % 4 != 1:                  # a few short columns stay clean
            bad.append(c)
        cols.append((_rows(rng, nf, n), p))
    case = SelCase("long", nf, cols, rs, bad)
    case.ties, case.where = tie_of, where
    ml = default_long(case.nnz, case.nc)
    assert ml == 4096 and case.nnz // case.nc <= 256
    badlen = case.col_len[case.bad]
    assert sorted(badlen[badlen > ml].tolist()) == [4097, 6000]
    assert (badlen > 8).sum() >= 257 + 6 and (badlen <= 8).sum() >= 50
    assert all(where[n] in case.bad for n in LONG_LENS)
    case.windows = [(0, case.nc), (where[4096], case.nc)]
    return case


def sel_cases():
    return [case_G(G) for G in (4, 8, 16, 32, 64)] + [case_long()]


# ------------------------------------------------------------------------------ expansion
def _rand_rows(rng, cn, lens):
    ro, cols = [0], []
    for n in lens:
        cols.extend(np.sort(rng.choice(cn, size=n, replace=False)).tolist())
        ro.append(len(cols))
    return Csr(len(lens), cn, np.array(ro, dtype=np.int64), np.array(cols, dtype=np.int64), np.ones(len(cols)))


@functools.lru_cache(maxsize=None)
def expand_cases():
    """(name, M, listed rows, fs_long settings): a matrix below nnz >= 16 rn (k_fs_expand, one
    thread per row), one above it with rows around the 64-lane strides (k_fs_expand_wave), and
    one with a 5 000-entry row among short ones (k_fs_expand_long); the lists hold duplicates"""
    rng = np.random.default_rng(11)
    out = []
    M = _rand_rows(rng, 500, rng.integers(0, 11, size=300).tolist())
    assert len(M.a) < 16 * M.rn
    out.append(("thread", M, np.concatenate([rng.choice(300, 90, replace=False), [5, 5, 17]]), (-1,)))
    lens = [63, 64, 65, 127, 128, 129, 1, 0, 8, 9] + rng.integers(10, 40, size=190).tolist()
    M = _rand_rows(rng, 3000, lens)
    assert len(M.a) >= 16 * M.rn
    out.append(("wave", M, np.concatenate([np.arange(10), rng.choice(200, 60, replace=False), [3, 3]]), (-1, 8)))
    lens = [5000] + rng.integers(1, 9, size=40).tolist() + rng.integers(9, 40, size=59).tolist()
    order = rng.permutation(100)
    M = _rand_rows(rng, 6000, [lens[q] for q in order])
    big = int(np.nonzero(order == 0)[0][0])
    assert len(M.a) >= 16 * M.rn and np.diff(M.row_off)[big] == 5000
    assert 5000 > max(4096, 16 * (len(M.a) // M.rn))       # long at the default threshold too
    out.append(("orphan", M, np.concatenate([[big], rng.choice(100, 50, replace=False), [big]]), (-1, 8)))
    return out


# ----------------------------------------------------------------------------- reductions
RED_FULL = 1024 * 256             # RED_BLOCKS x RED_THREADS: one full grid of partials
RED_N = (1, 255, 256, 257, RED_FULL - 1, RED_FULL, RED_FULL + 1, 3 * RED_FULL - 1, 3 * RED_FULL,
         3 * RED_FULL + 1)


def red_vectors(n):
    """(name, a): non-negative vectors of length n whose first maximum is known by design"""
    rng = np.random.default_rng(n)
    base = rng.integers(0, 1000, size=n) / 1024.0
    out = [("random", base.copy()), ("all_equal", np.full(n, 0.75))]
    a = base.copy(); a[n - 1] = 2.0
    out.append(("max_last", a))
    if n >= 257:
        a = base.copy(); a[[n - 1, 256, 200, 130]] = 2.0            # twice in block 0, and in later blocks
        out.append(("repeated", a))
    if n >= 1024:
        a = base.copy(); a[[n - 1, n - 256 - 3]] = 2.0               # two different blocks, none early
        out.append(("two_blocks", a))
    if n > RED_FULL:
        a = base.copy(); a[[RED_FULL, 256]] = 2.0                    # block 0 on its second stride against block 1
        out.append(("strides", a))
    return out


# ------------------------------------------------------------------------------ whole loop
@functools.lru_cache(maxsize=None)
def loop_orphan():
    """nf 6000, nc 1500: 6 entries k/64 (k 1..15) per row in columns 1.., and column 0 with
    5 000 entries k/64 (k 1..3).  Every sum is exact.  goal = 0.9 x the first max(w2 ./ w)."""
    rng = np.random.default_rng(3)
    nf, nc = 6000, 1500
    in0 = np.zeros(nf, dtype=bool)
    in0[rng.choice(nf, 5000, replace=False)] = True
    ro, cols, vals = [0], [], []
    for i in range(nf):
        c = np.sort(rng.choice(nc - 1, size=6, replace=False) + 1).tolist()
        v = (rng.integers(1, 16, size=6) / 64.0).tolist()
        if in0[i]:
            c, v = [0] + c, [float(rng.integers(1, 4)) / 64.0] + v
        cols.extend(c); vals.extend(v); ro.append(len(cols))
    R = Csr(nf, nc, np.array(ro, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals))
    first = refops.fs_products(R, refops.Csc(R), R.a)
    with np.errstate(divide="ignore", invalid="ignore"):
        mv = float(np.where(first[1] == 0.0, 0.0, first[3] / first[1]).max())
    return R, 0.9 * mv


@functools.lru_cache(maxsize=None)
def loop_banded():
    """nf 3000, nc 700, 8 entries per row within a band of 41 columns, general values.  Twelve
    adjacent columns are 5 x heavier and six far from them 3 x: while only the first cluster
    is bad the three expansions stay within the caps (the incremental path); sweeps in which
    both are bad overflow a cap and fall back to full products.  6-18 short bad
    columns per sweep.  The sweep counts are checked by test_fs_cases_cpu.py."""
    rng = np.random.default_rng(5)
    nf, nc, half = 3000, 700, 20
    ro, cols, vals = [0], [], []
    for i in range(nf):
        ctr = min(max(int(round(i * (nc - 1) / (nf - 1))), half), nc - 1 - half)
        c = np.sort(rng.choice(2 * half + 1, size=8, replace=False) + ctr - half)
        cols.extend(c.tolist()); vals.extend(rng.uniform(0.05, 1.0, size=8).tolist()); ro.append(len(cols))
    cols, vals = np.array(cols, dtype=np.int64), np.array(vals)
    vals[(cols >= 335) & (cols < 347)] *= 5.0
    vals[(cols >= 600) & (cols < 606)] *= 3.0
    R = Csr(nf, nc, np.array(ro, dtype=np.int64), cols, vals)
    first = refops.fs_products(R, refops.Csc(R), R.a)
    mv = float((first[3] / first[1]).max())
    return R, LOOP_BANDED_FACTOR * mv


LOOP_BANDED_FACTOR = 0.3


def loop_tiny():
    """nf = 2: a goal the loop reaches by selecting, and one above the first max(v) (no
    selection, an empty skeleton)"""
    R = Csr(2, 3, np.array([0, 3, 5], dtype=np.int64), np.array([0, 1, 2, 0, 2], dtype=np.int64),
            np.array([0.5, 0.25, 1.0, 0.75, 0.125]))
    return R


def oracle_find_support(lib, R, goal):
    """the oracle's own find_support (oracle/amg_oracle.c, exported for the tests): a second
    reference with the reference's summation order at C speed.  Returns (Sk, sweeps, UB events)"""
    import ctypes as C
    f = lib.oracle_find_support
    f.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    f.restype = C.c_int
    ro = np.ascontiguousarray(R.row_off, dtype=np.uint64)
    col = np.ascontiguousarray(R.col, dtype=np.uint32)
    a = np.ascontiguousarray(R.a, dtype=np.float64)
    cap = len(a) + R.cn + 16
    oro, ocol, oa_ = np.zeros(R.rn + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap)
    info = np.zeros(3, dtype=np.uint64)
    rc = f(R.rn, R.cn, ro.ctypes.data, col.ctypes.data, a.ctypes.data, float(goal), oro.ctypes.data,
           ocol.ctypes.data, oa_.ctypes.data, cap, info.ctypes.data)
    assert rc == 0, rc
    n = int(info[0])
    return Csr(R.rn, R.cn, oro.astype(np.int64), ocol[:n].astype(np.int64), oa_[:n].copy()), int(info[1]), int(info[2])
