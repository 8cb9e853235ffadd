"""Inputs of the row-partitioned primitive tests (tests/test_gpu_part_prims.py).

Pure numpy and seeded: every rank of a launch generates identical inputs.  A partition is a
split array of N + 1 entries; the kinds are ones no grid setup produces:

  even       n * p // N (apart_even's)
  ragged     random cut points
  empty      ranks 0, N // 2 and N - 1 own no rows, the others get ragged cuts.  With N <= 3
             those three ranks are all of them, so the middle rank keeps the rows (N = 3:
             ranks 0 and 2 empty; N = 2: rank 0 empty)
  one_owner  every row on the last rank

Each case builder asserts the property the case exists for (`need`), so a change of sizes
or seeds cannot silently turn a case into an ordinary one; tests/test_part_cases_cpu.py runs
every builder for every launch of the GPU test.  The `model_*` functions restate each exchange
on host blocks (per-rank transposes concatenated in rank order, the halo view, the stable
route by owner) for the CPU test to compare with the whole-matrix refops result.
"""
import numpy as np

import refops
from refops import Csr

KINDS = ("even", "ragged", "empty", "one_owner")
# (N, kind) of every launch of test_gpu_part_prims.py
LAUNCHES = [(N, k) for N in (2, 3, 4) for k in KINDS] + [(8, "ragged"), (8, "empty")]


def need(cond, what):
    assert cond, "case lost its property: " + what


# ------------------------------------------------------------------ partitions
def empty_ranks(N):
    e = {0, N // 2, N - 1}
    if len(e) >= N:
        e.discard(N // 2 if N == 3 else N - 1)
    return sorted(e)


def split(kind, n, N, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "even":
        s = [n * p // N for p in range(N + 1)]
    elif kind == "ragged":
        while True:
            s = [0] + sorted(rng.integers(1, n, N - 1).tolist()) + [n]
            if s != [n * p // N for p in range(N + 1)] and len(set(np.diff(s))) > 1:
                break
    elif kind == "empty":
        own = [p for p in range(N) if p not in empty_ranks(N)]
        cuts = [0] + sorted(rng.integers(1, n, len(own) - 1).tolist()) + [n]
        while len(set(cuts)) != len(cuts):
            cuts = [0] + sorted(rng.integers(1, n, len(own) - 1).tolist()) + [n]
        s, k = [0], 0
        for p in range(N):
            if p in own:
                k += 1
            s.append(cuts[k])
        need(all(s[p] == s[p + 1] for p in empty_ranks(N)), "empty ranks")
    elif kind == "one_owner":
        s = [0] * N + [n]
    else:
        raise ValueError(kind)
    s = np.array(s, dtype=np.int64)
    need(s[0] == 0 and s[-1] == n and np.all(np.diff(s) >= 0) and len(s) == N + 1, "a split")
    return s


def owners(s):
    """ranks that own at least one row"""
    return [p for p in range(len(s) - 1) if s[p + 1] > s[p]]


def owner_of(s, i):
    return int(np.searchsorted(s, i, side="right") - 1)


# ------------------------------------------------------------------ CSR helpers
def from_rows(rows, cn):
    """rows: list of (cols, vals); columns kept in the given order (ascending, repeats allowed)"""
    ro, cols, vals = [0], [], []
    for c, v in rows:
        need(len(c) == len(v) and all(c[k] <= c[k + 1] for k in range(len(c) - 1)), "ascending columns")
        cols.extend(int(x) for x in c)
        vals.extend(float(x) for x in v)
        ro.append(len(cols))
    return Csr(len(rows), cn, np.array(ro, dtype=np.int64), np.array(cols, dtype=np.int64),
               np.array(vals, dtype=np.float64))


def to_rows(A):
    return [(A.col[A.row_off[i]:A.row_off[i + 1]].tolist(), A.a[A.row_off[i]:A.row_off[i + 1]].tolist())
            for i in range(A.rn)]


def block(A, lo, hi):
    """rows [lo, hi) of A as a local block (global columns)"""
    k0, k1 = int(A.row_off[lo]), int(A.row_off[hi])
    return Csr(hi - lo, A.cn, np.asarray(A.row_off[lo:hi + 1], dtype=np.int64) - k0,
               np.asarray(A.col[k0:k1], dtype=np.int64), None if A.a is None else np.asarray(A.a[k0:k1]))


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def diff_csr(X, Y, vals=True, cols=True):
    """None when the blocks are identical bit for bit, else the first differing row / entry"""
    if X is None:
        return "no output"
    if (X.rn, X.cn) != (Y.rn, Y.cn):
        return f"shape {(X.rn, X.cn)} != {(Y.rn, Y.cn)}"
    xr, yr = np.asarray(X.row_off, dtype=np.int64), np.asarray(Y.row_off, dtype=np.int64)
    if not np.array_equal(xr, yr):
        i = int(np.nonzero(xr != yr)[0][0])
        return f"row offsets differ first at {i}: {int(xr[i])} != {int(yr[i])}"
    for name, on, x, y in (("col", cols, X.col, Y.col), ("a", vals, X.a, Y.a)):
        if not on:
            continue
        if x is None:
            return f"{name} missing"
        x, y = (np.asarray(x), np.asarray(y)) if name == "col" else (bits(x), bits(y))
        if len(x) != len(y):
            return f"{name} length {len(x)} != {len(y)}"
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            i = int(np.searchsorted(xr, k, side="right") - 1)
            gx, gy = (X.col[k], Y.col[k]) if name == "col" else (X.a[k], Y.a[k])
            return f"{name} differs first at entry {k} (row {i}): {gx!r} != {gy!r}"
    return None


def diff_vec(x, y):
    x, y = bits(x), bits(y)
    if len(x) != len(y):
        return f"length {len(x)} != {len(y)}"
    if np.array_equal(x, y):
        return None
    i = int(np.nonzero(x != y)[0][0])
    return f"differs first at {i}: {x[i:i + 1].view(np.float64)[0]!r} != {y[i:i + 1].view(np.float64)[0]!r}"


def positive(A):
    return Csr(A.rn, A.cn, A.row_off, A.col, np.abs(A.a) + 0.25)


def with_row_lengths(rng, rn, cn, lens):
    rows = []
    for i in range(rn):
        k = min(int(lens[i]), cn)
        c = np.sort(rng.choice(cn, size=k, replace=False))
        rows.append((c.tolist(), rng.standard_normal(k).tolist()))
    return from_rows(rows, cn)


# ------------------------------------------------------------------ host models of the exchanges
def model_transpose(A, rs, cs):
    """pm_transpose restated on host blocks: rank q transposes its rows; the owner of column j
    concatenates the pieces of row j of A^T in rank order.  Returns the whole A^T."""
    N = len(rs) - 1
    pieces = []
    for q in range(N):
        T = refops.transpose(block(A, rs[q], rs[q + 1]))         # columns are local rows
        pieces.append(T)
    rows = []
    for j in range(A.cn):
        c, v = [], []
        for q in range(N):
            T = pieces[q]
            s, e = T.row_off[j], T.row_off[j + 1]
            c.extend((np.asarray(T.col[s:e]) + rs[q]).tolist())
            v.extend(np.asarray(T.a[s:e]).tolist())
        rows.append((c, v))
    return from_rows(rows, A.rn)


def model_halo(B, bs, me, Lcols):
    """pm_halo_rows restated: B's own rows and the rows referenced by Lcols, in a global-row
    view (every other row empty)"""
    want = set(int(c) for c in Lcols) | set(range(int(bs[me]), int(bs[me + 1])))
    rows = to_rows(B)
    return from_rows([rows[i] if i in want else ([], []) for i in range(B.rn)], B.cn)


def model_route(I, J, V, parts, s):
    """pm_route_coo restated: parts = per-rank (k0, k1) ranges of the concatenated entries;
    returns per owner (I, J, V): the entries in source-rank order, then original position"""
    out = []
    for p in range(len(s) - 1):
        sel = [k for (k0, k1) in parts for k in range(k0, k1) if s[p] <= I[k] < s[p + 1]]
        out.append((I[sel], J[sel], V[sel]))
    return out


def rowsums(A):
    return refops.spmv(A, np.ones(A.cn))


# ------------------------------------------------------------------ cases
def case_induced(N, kind, seed):
    n = 300
    s = split(kind, n, N, seed)
    rng = np.random.default_rng(seed)
    out = [("random", s, (rng.random(n) < 0.4).astype(np.uint8)), ("all_zero", s, np.zeros(n, dtype=np.uint8))]
    m = (rng.random(n) < 0.6).astype(np.uint8)
    p = owners(s)[0]
    m[s[p]:s[p + 1]] = 0
    m[s[owners(s)[-1] + 1] - 1] = 1 if len(owners(s)) > 1 else 0
    need(not m[s[p]:s[p + 1]].any(), "mask empty on one owning rank")
    out.append(("empty_on_one", s, m))
    return out


def ref_induced(s, mask):
    return np.concatenate([[0], np.cumsum(mask.astype(np.int64))])[s]


def case_transpose(N, kind, seed):
    """(name, A, rs, cs)"""
    rng = np.random.default_rng(seed)
    out = []
    # rectangular, independent row and column partitions
    rn, cn = 320, 217
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    A = refops.rand_csr(rng, rn, cn, 0.03)
    need(rn != cn and not np.array_equal(rs, cs), "row partition != column partition")
    out.append(("rect", A, rs, cs))
    # long columns fed by every owning rank, a repeated column within a row
    rows = to_rows(refops.rand_csr(rng, rn, cn, 0.02))
    src = owners(rs)
    for i in range(rn):
        c, v = rows[i]
        keep = [(x, y) for x, y in zip(c, v) if x > 2]
        add = [(0, rng.standard_normal())] if i % 4 == 0 or i in [rs[p] for p in src] else []
        add += [(1, rng.standard_normal())] if i % 8 != 7 or i in [rs[p] for p in src] else []
        if i % 16 == 3:
            add += [(2, 1.5), (2, -0.5)]                      # the same column twice in one row
        rows[i] = ([x for x, _ in add + keep], [y for _, y in add + keep])
    A = from_rows(rows, cn)
    cnt = np.bincount(A.col, minlength=cn)
    need(64 < cnt[0] <= 256 < cnt[1], f"columns of > 64 and > 256 entries ({cnt[0]}, {cnt[1]})")
    for j in (0, 1):
        r = np.nonzero([j in rows[i][0] for i in range(rn)])[0]
        need(set(owner_of(rs, i) for i in r) == set(src), "a long column drawn from every owning rank")
    need(any(len(set(c)) < len(c) for c, _ in rows), "a repeated column within a row")
    out.append(("long_cols", A, rs, cs))
    # every entry lands on one rank
    q = max(owners(cs), key=lambda p: cs[p + 1] - cs[p])
    rows = []
    for i in range(rn):
        k = int(rng.integers(0, 5))
        c = np.sort(rng.choice(np.arange(cs[q], cs[q + 1]), size=min(k, cs[q + 1] - cs[q]), replace=False))
        rows.append((c.tolist(), rng.standard_normal(len(c)).tolist()))
    A = from_rows(rows, cn)
    need(A.row_off[-1] > 0 and all(owner_of(cs, c) == q for c in A.col), "every entry on one rank")
    out.append(("one_dest", A, rs, cs))
    # empty ranks on the source side only / on the destination side only
    A = refops.rand_csr(rng, rn, cn, 0.03)
    e_r, v_c = split("empty", rn, N, seed + 2), split("even", cn, N)
    need(len(owners(e_r)) < N and len(owners(v_c)) == N, "empty source ranks, full destination")
    out.append(("src_empty", A, e_r, v_c))
    v_r, e_c = split("even", rn, N), split("empty", cn, N, seed + 3)
    need(len(owners(v_r)) == N and len(owners(e_c)) < N, "full source, empty destination ranks")
    out.append(("dst_empty", A, v_r, e_c))
    return out


def case_spgemm(N, kind, seed):
    """(name, A, B, rs (A rows), ms (A columns = B rows), ks (B columns))"""
    rng = np.random.default_rng(seed + 50)
    out = []
    n, m, k = 260, 231, 190
    rs, ms, ks = split(kind, n, N, seed), split(kind, m, N, seed + 1), split(kind, k, N, seed + 2)
    B = to_rows(refops.rand_csr(rng, m, k, 0.04, minrow=1))
    bown = owners(ms)
    hub = int(ms[bown[-1] + 1] - 1)                      # one B row needed by every rank
    firsts = [int(ms[q]) for q in bown]                   # a row of every B owner
    empt = [int(ms[q + 1] - 1) for q in bown if ms[q + 1] - ms[q] >= 3]   # empty B rows, requested
    empt = [j for j in empt if j != hub and j not in firsts]
    for j in empt:
        B[j] = ([], [])
    B = from_rows(B, k)
    A = to_rows(refops.rand_csr(rng, n, m, 0.02))
    for p in owners(rs):
        i = int(rs[p])
        c = sorted(set(firsts + [hub] + empt + A[i][0]))
        A[i] = (c, rng.standard_normal(len(c)).tolist())
    A = from_rows(A, m)
    for p in owners(rs):
        ref = set(owner_of(ms, c) for c in block(A, rs[p], rs[p + 1]).col)
        need(ref >= set(bown), "A references rows of every B owner from every rank")
        cols = set(block(A, rs[p], rs[p + 1]).col.tolist())
        need(hub in cols, "one B row needed by all ranks")
        need(not empt or set(empt) <= cols, "empty B rows requested")
    if len(bown) >= 3:
        q = bown[1]
        need(firsts[0] < ms[q] and hub >= ms[q + 1], "needed rows below and above the own range")
    out.append(("all_ranks", A, B, rs, ms, ks))
    # block diagonal: no rank needs another's rows
    n2 = 240
    s2 = split(kind, n2, N, seed + 4)
    rows = []
    for i in range(n2):
        p = owner_of(s2, i)
        cnt = min(int(rng.integers(1, 6)), s2[p + 1] - s2[p])
        c = np.sort(rng.choice(np.arange(s2[p], s2[p + 1]), size=cnt, replace=False))
        rows.append((c.tolist(), rng.standard_normal(cnt).tolist()))
    A2 = from_rows(rows, n2)
    need(all(owner_of(s2, c) == owner_of(s2, i) for i in range(n2) for c in rows[i][0]), "block diagonal: nneed == 0")
    out.append(("block_diag", A2, refops.rand_csr(rng, n2, k, 0.04), s2, s2, ks))
    # own block empty on some ranks (A and B), whatever the launch's kind
    e_r, e_m = split("empty", n, N, seed + 5), split("empty", m, N, seed + 6)
    need(len(owners(e_r)) < N and len(owners(e_m)) < N, "own block empty")
    out.append(("own_empty", A, B, e_r, e_m, ks))
    return out


def case_sub_mat(N, kind, seed):
    """(name, A, rs, cs, vr, vc)"""
    rng = np.random.default_rng(seed + 60)
    rn, cn = 300, 260
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    own = owners(rs)
    lens = np.array([24 if owner_of(rs, i) == own[0] else 6 for i in range(rn)])
    if len(own) == 1:                                   # one block: half long rows, mean below 16
        lens[rs[own[0]]:rs[own[0] + 1]] = 6
    A = with_row_lengths(rng, rn, cn, lens)
    means = [block(A, rs[p], rs[p + 1]).row_off[-1] / (rs[p + 1] - rs[p]) for p in own]
    need(len(own) == 1 or (max(means) > 16 > min(means)), f"block mean row lengths straddle 16: {means}")
    vr, vc = (rng.random(rn) < 0.5).astype(np.uint8), (rng.random(cn) < 0.5).astype(np.uint8)
    out = [("straddle16", A, rs, cs, vr, vc)]
    vr2 = vr.copy()
    p = own[-1]
    vr2[rs[p]:rs[p + 1]] = 0
    need(not vr2[rs[p]:rs[p + 1]].any(), "all rows masked out on one rank")
    out.append(("rank_masked_out", A, rs, cs, vr2, vc))
    return out


def ref_sub_mat(A, vr, vc):
    cmap = np.cumsum(vc.astype(np.int64)) - 1
    rows = []
    for i, (c, v) in enumerate(to_rows(A)):
        if vr[i]:
            rows.append(([int(cmap[x]) for x in c if vc[x]], [y for x, y in zip(c, v) if vc[x]]))
    return from_rows(rows, int(vc.sum()))


def case_vec(N, kind, seed):
    """square A (rows and columns split alike) for the vector-valued ops and diag ops"""
    rng = np.random.default_rng(seed + 70)
    n = 280
    s = split(kind, n, N, seed)
    own = owners(s)
    lens = np.array([40 if owner_of(s, i) == own[0] else 7 for i in range(n)])
    if len(own) == 1:
        lens[:] = np.where(np.arange(n) % 2, 7, 40)
    rows = to_rows(with_row_lengths(rng, n, n, lens))
    for i in range(n):                                  # a diagonal everywhere ...
        c, v = rows[i]
        if i not in c:
            k = int(np.searchsorted(c, i))
            c.insert(k, i); v.insert(k, float(rng.standard_normal()))
    miss = [int(s[p]) + (int(s[p + 1] - s[p]) // 2) for p in own]     # ... but missing in these rows
    twice = [int(s[p + 1]) - 1 for p in own if s[p + 1] - s[p] > 2]     # and stored twice in these
    for i in miss:
        c, v = rows[i]
        k = c.index(i); del c[k]; del v[k]
    for i in twice:
        c, v = rows[i]
        k = c.index(i); c.insert(k, i); v.insert(k, float(rng.standard_normal()))
    A = from_rows(rows, n)
    means = [block(A, s[p], s[p + 1]).row_off[-1] / (s[p + 1] - s[p]) for p in own]
    need(len(own) == 1 or (max(means) >= 32 > min(means)), f"SpMV kernels differ per rank: {means}")
    need(all(i not in rows[i][0] for i in miss) and miss, "diagonal missing in a row")
    need(all(rows[i][0].count(i) == 2 for i in twice) and (twice or len(own) == 1 and n < 3),
         "diagonal stored twice in a row")
    return A, s


def ref_diag(A):
    D = np.zeros(A.rn)
    for i, (c, v) in enumerate(to_rows(A)):
        if i in c:
            D[i] = v[c.index(i)]                        # the first stored diagonal
    return D


def ref_rowsum_sq_inv(A):
    out = np.zeros(A.rn)
    with np.errstate(all="ignore"):
        for i, (_, v) in enumerate(to_rows(A)):
            t = 0.0
            for x in v:
                t += x * x
            out[i] = np.float64(1.0) / np.float64(t)
    return out


def ref_diag_op(A, Dl, Dr, op):
    """amgd_diag_op / amgd_diag_op2 (diagcsr_op's passes): 0 DPLUS, 1 DMINUS (the first stored
    diagonal only), 2 DMULT, 3 MULTD, 4 SCALE2, 5 SCALE_ABS, 6 SCALE2_ABS, 7 SCALE_ABS_T"""
    rows = to_rows(A)
    for i, (c, v) in enumerate(rows):
        if op in (0, 1):
            if i in c:
                k = c.index(i)
                v[k] = v[k] + Dl[i] if op == 0 else v[k] - Dl[i]
            continue
        for k, j in enumerate(c):
            a = v[k]
            v[k] = {2: lambda: a * Dl[i], 3: lambda: a * Dl[j], 4: lambda: (a * Dl[i]) * Dr[j],
                    5: lambda: abs(a * Dl[i]) * Dr[j], 6: lambda: abs((a * Dl[i]) * Dr[j]),
                    7: lambda: abs(a * Dl[j]) * Dr[i]}[op]()
    return from_rows(rows, A.cn)


def ref_spmv_f(A, x, alpha, y, beta, f):
    z = refops.spmv(A, x, alpha, y, beta)
    return z if f is None else z * np.where(f != 0, 1.0, 0.0)


def case_rowops(N, kind, seed):
    """A, B on the same partitions for mpm / mxmpoint / drop_zeros / rows_masked; one rank's
    block empty (an owning rank whose rows hold no entries, beside the ranks without rows)"""
    rng = np.random.default_rng(seed + 80)
    rn, cn = 250, 200
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    A, B = to_rows(refops.rand_csr(rng, rn, cn, 0.04, ints=True)), to_rows(refops.rand_csr(rng, rn, cn, 0.04, ints=True))
    p = owners(rs)[0]
    if len(owners(rs)) > 1:
        for i in range(rs[p], rs[p + 1]):
            A[i] = ([], [])
    for i in range(0, rn, 3):                           # exact zeros to drop
        if A[i][1]:
            A[i][1][0] = 0.0
    A, B = from_rows(A, cn), from_rows(B, cn)
    need(len(owners(rs)) < N or block(A, rs[p], rs[p + 1]).row_off[-1] == 0, "one rank's block empty")
    mask = (rng.random(rn) < 0.5).astype(np.uint8)
    return A, B, rs, cs, mask


def ref_drop_zeros(A):
    return from_rows([([x for x, y in zip(c, v) if y != 0.0], [y for y in v if y != 0.0]) for c, v in to_rows(A)], A.cn)


def ref_rows_masked(A, mask):
    return from_rows([(c, v) if mask[i] else ([], []) for i, (c, v) in enumerate(to_rows(A))], A.cn)


def case_list_sync(N, kind, seed, rank):
    """(name, vectors): vectors = [(s, owner values, this rank's list, this rank's start vector)];
    every rank holds the same list content in its own order and pre-fills the entries it does
    not own with a rank-specific sentinel"""
    out = []
    rng = np.random.default_rng(seed + 90)
    for name, n, pick in (("front", 300, "random"), ("one_owner_rows", 300, "one"), ("empty_list", 300, "none"),
                          ("second_space", 211, "random")):
        s = split(kind, n, N, seed + (7 if name == "second_space" else 0))
        truth = rng.standard_normal(n)
        if pick == "random":
            lst = rng.choice(n, size=131 if n == 300 else 77, replace=False)
        elif pick == "one":
            p = max(owners(s), key=lambda q: s[q + 1] - s[q])
            lst = np.arange(s[p], s[p + 1])[:97]
            need(len(set(owner_of(s, i) for i in lst)) == 1, "all listed rows owned by one rank")
        else:
            lst = np.zeros(0, dtype=np.int64)
        need(name == "empty_list" or len(lst) % 64 != 0, "list length not a multiple of 64")
        mine = np.random.default_rng(seed + 17 * rank + 1).permutation(lst)     # this rank's order
        other = np.random.default_rng(seed + 17 * (rank + 1) + 1).permutation(lst)
        need(len(lst) < 2 or not np.array_equal(mine, other), "each rank holds the list in a different order")
        z0 = np.full(n, -1000.0 - rank)
        z0[s[rank]:s[rank + 1]] = truth[s[rank]:s[rank + 1]]
        want = z0.copy()
        want[lst] = truth[lst]
        out.append((name, s, mine.astype(np.uint32), z0, want))
    return out


def adversarial_rows(rng, rn, cn, short):
    """rows with cancellation and mixed magnitudes (the kinds of test_gpu_kernels'
    _adversarial_rows, nan / inf left out: the comparison is bit for bit)"""
    kinds = ["pos", "ties", "zeros", "cancel", "sub", "huge", "hover", "mixed"]
    rows = []
    for i in range(rn):
        kind = kinds[i % len(kinds)]
        L = int(rng.choice([1, 2, 5, 9] if short[i] else [63, 64, 65, 130]))
        if kind == "pos":
            v = np.abs(rng.standard_normal(L)) * 2.0 ** rng.integers(-3, 4, L)
        elif kind == "ties":
            v = np.where(rng.random(L) < 0.5, 2.0 ** -53, 1.0) * (1 + (rng.random(L) < 0.3))
            v[0] = 1.0
        elif kind == "zeros":
            v = np.where(rng.random(L) < 0.6, 0.0, rng.standard_normal(L))
            v[: L // 2] = -0.0
        elif kind == "cancel":
            h = rng.standard_normal((L + 1) // 2)
            v = np.concatenate([h, -h])[:L]
        elif kind == "sub":
            v = rng.standard_normal(L) * 2.0 ** -1070
        elif kind == "huge":
            v = rng.standard_normal(L) * 2.0 ** rng.integers(900, 1000, L)
        elif kind == "hover":
            v = np.where(rng.random(L) < 0.5, 1.0, -1.0) * 2.0 ** -52
            v[0] = 1.0
        else:
            v = rng.standard_normal(L) * 10.0 ** rng.integers(-12, 12, L)
        c = np.sort(rng.choice(cn, size=L, replace=False))
        rows.append((c.tolist(), v.tolist()))
    return from_rows(rows, cn)


def case_list_rowsum(N, kind, seed):
    """A (n x cn) and B (m x cn): blocks on both sides of the nnz > 32 * rn switch"""
    rng = np.random.default_rng(seed + 100)
    out = []
    for n, sd in ((240, 0), (200, 9)):
        s = split(kind, n, N, seed + sd)
        own = owners(s)
        short = np.array([owner_of(s, i) != own[0] for i in range(n)])
        if len(own) == 1:
            short[:] = bool(sd)                          # one block: A long rows, B short rows
        M = adversarial_rows(rng, n, 400, short)
        side = [block(M, s[p], s[p + 1]).row_off[-1] > 32 * (s[p + 1] - s[p]) for p in own]
        out.append((M, s, side))
    need(any(x for _, _, sd in out for x in sd) and any(not x for _, _, sd in out for x in sd),
         "blocks on both sides of the nnz > 32 rn switch")
    la = rng.choice(out[0][0].rn, size=150, replace=False).astype(np.uint32)
    lb = rng.choice(out[1][0].rn, size=150, replace=False).astype(np.uint32)
    return out[0][:2], out[1][:2], la, lb


def eager_shares(N, rank, slot=4096):
    """the byte counts of the eager sequence on one persistent state, per call and rank: the
    largest share grows, then shrinks; shares of 0, 1, 7, slot, slot + 1, 3 MB + 5"""
    big = 3 * 1024 * 1024 + 5
    calls = [[0] * N,                                                     # every share empty
             [(0, 1, 7)[p % 3] for p in range(N)],
             [slot if p == 0 else slot + 1 if p == 1 else 7 for p in range(N)],   # second round by 1 byte
             [slot if p % 2 else 1 for p in range(N)],
             [7] * N,
             [big if p == N - 1 else 0 for p in range(N)],              # grows: slot -> 1 MB cap
             [20000 * (p + 1) for p in range(N)]]                        # shrinks, still above the default
    need({0, 1, 7, slot, slot + 1, big} <= set(x for c in calls for x in c), "eager share sizes")
    return calls


def eager_payload(call, p, nbytes):
    return np.random.default_rng(10_000 + 97 * call + p).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


def eager_expect_slots(calls, forced=0):
    """slot used by each call and whether it takes the second round (pm_allgather_dyn's rule:
    first 4096, afterwards 5/4 of the previous call's largest share within [4 KB, 1 MB])"""
    slot, out = 4096, []
    for c in calls:
        use = max(8, forced) if forced else slot
        use = (use + 7) & ~7
        out.append((use, any(x > use for x in c)))
        mx = max(c)
        slot = min(max(mx + mx // 4, 4096), 1 << 20)
    return out


def case_route(N, kind, seed):
    """whole COO and each rank's contiguous share of it"""
    rng = np.random.default_rng(seed + 110)
    n = 300
    s = split(kind, n, N, seed)
    nz = 900
    I, J = rng.integers(0, n, nz), rng.integers(0, n, nz)
    cutp = [0] + sorted(rng.integers(0, nz, N - 1).tolist()) + [nz]
    z = 1 if N > 2 else 0                                # a rank passing zero entries
    cutp[z + 1] = cutp[z]
    cutp = sorted(cutp)
    parts = [(cutp[p], cutp[p + 1]) for p in range(N)]
    need(any(a == b for a, b in parts), "a rank passing zero entries")
    srcs = [p for p, (a, b) in enumerate(parts) if b - a >= 4]
    a0 = parts[srcs[0]][0]
    I[a0 + 1], J[a0 + 1] = I[a0], J[a0]                  # duplicate within one rank
    I[a0 + 3], J[a0 + 3] = I[a0], J[a0]
    if len(srcs) > 1:
        b0 = parts[srcs[-1]][0]
        I[b0 + 2], J[b0 + 2] = I[a0], J[a0]              # and on another rank
    V = rng.standard_normal(nz)
    key = list(zip(I.tolist(), J.tolist()))
    need(key[a0:parts[srcs[0]][1]].count(key[a0]) >= 3, "duplicate (i, j) within one rank")
    need(len(srcs) == 1 or key[a0] in key[parts[srcs[-1]][0]:parts[srcs[-1]][1]], "duplicate (i, j) on different ranks")
    out = [("dups", I, J, V, parts, s)]
    p = owners(s)[-1]
    I2 = rng.integers(s[p], s[p + 1], nz)
    need(all(owner_of(s, i) == p for i in I2), "every entry going to one owner")
    out.append(("one_owner_dest", I2, J, V, parts, s))
    return out


def case_kpos(N, kind, seed):
    """W_skel-like matrix: a few columns whose supports span several ranks"""
    rng = np.random.default_rng(seed + 120)
    rn, cn = 300, 40
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    rows = [(np.sort(rng.choice(cn, size=int(rng.integers(0, 3)), replace=False)).tolist(),) for _ in range(rn)]
    A = from_rows([(c[0], [1.0] * len(c[0])) for c in rows], cn)
    if len(owners(rs)) > 1:
        T = refops.transpose(A)
        need(any(len(set(owner_of(rs, i) for i in T.col[T.row_off[j]:T.row_off[j + 1]])) > 1 for j in range(cn)),
             "supports spanning several ranks")
    return A, rs, cs


def ref_kpos(A):
    T = refops.transpose(A)
    out = np.zeros(len(A.col))
    for i in range(A.rn):
        for e in range(A.row_off[i], A.row_off[i + 1]):
            j = A.col[e]
            out[e] = T.col[T.row_off[j]:T.row_off[j + 1]].tolist().index(i)
    return out


def case_zero_entries(N, kind, seed):
    rng = np.random.default_rng(seed + 130)
    rn, cn = 260, 220
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    A = refops.rand_csr(rng, rn, cn, 0.05, minrow=1)
    ks = rng.choice(len(A.col), size=120, replace=False)
    ri = (np.searchsorted(A.row_off, ks, side="right") - 1).astype(np.int64)
    cj = A.col[ks]
    ri, cj = np.concatenate([ri, ri[:5]]), np.concatenate([cj, cj[:5]])       # pairs listed twice
    need(len(set(zip(ri.tolist(), cj.tolist()))) < len(ri), "a pair listed twice")
    need(len(owners(rs)) == 1 or len(set(owner_of(rs, i) for i in ri)) > 1, "pairs owned by other ranks")
    return A, rs, cs, ri, cj


def ref_zero_entries(A, ri, cj):
    rows = to_rows(A)
    for i, j in zip(ri, cj):
        c, v = rows[i]
        v[c.index(j)] = 0.0
    return from_rows(rows, A.cn)


def case_coo_ones(N, kind, seed):
    rng = np.random.default_rng(seed + 140)
    rn, cn = 240, 200
    rs, cs = split(kind, rn, N, seed), split(kind, cn, N, seed + 1)
    ri, cj = rng.integers(0, rn, 700), rng.integers(0, cn, 700)
    ri[100], cj[100] = ri[5], cj[5]                      # a repeated pair
    i = int(ri[0])
    at = np.nonzero(ri == i)[0]
    need(len(at) > 1 and np.any(np.diff(at) > 1), "entries of one row scattered through the list")
    need(len(set(zip(ri.tolist(), cj.tolist()))) < len(ri), "a repeated pair")
    return rs, cs, ri, cj
