"""The inputs of the row-partitioned primitive tests, checked without a GPU: every case of
tests/part_cases.py keeps the property it exists for (the builders assert them) at every
(ranks, partition kind, seed) the GPU test launches, and a numpy model of each exchange --
per-rank transposes concatenated in rank order, the assembled halo view, the stable route by
owner -- equals the whole-matrix refops result the GPU test compares against."""
import numpy as np
import pytest

import part_cases as pc
import refops

SEEDS = (0, 1, 2)          # part_prim_worker.SEEDS
IDS = [f"{N}-{k}" for N, k in pc.LAUNCHES]


@pytest.mark.parametrize("N,kind", pc.LAUNCHES, ids=IDS)
def test_partitions(N, kind):
    for n in (200, 300, 3000):
        for sd in SEEDS:
            s = pc.split(kind, n, N, sd)
            sizes = np.diff(s)
            if kind == "even":
                assert sizes.max() - sizes.min() <= 1
            elif kind == "ragged":
                assert len(set(sizes.tolist())) > 1
            elif kind == "empty":
                assert all(sizes[p] == 0 for p in pc.empty_ranks(N)) and sizes.sum() == n
                assert {0, N - 1} & set(pc.empty_ranks(N)) and (N < 4 or len(pc.empty_ranks(N)) == 3)
            else:
                assert sizes[-1] == n and not sizes[:-1].any()
            assert [pc.owner_of(s, i) for i in (0, n - 1)] == [pc.owners(s)[0], pc.owners(s)[-1]]


@pytest.mark.parametrize("N,kind", pc.LAUNCHES, ids=IDS)
def test_cases_keep_their_properties(N, kind):
    """every builder runs (and asserts its property) for every seed of the launch"""
    for sd in SEEDS:
        pc.case_induced(N, kind, sd)
        pc.case_transpose(N, kind, sd)
        pc.case_spgemm(N, kind, sd)
        pc.case_sub_mat(N, kind, sd)
        pc.case_vec(N, kind, sd)
        pc.case_rowops(N, kind, sd)
        for me in range(N):
            pc.case_list_sync(N, kind, sd, me)
        pc.case_list_rowsum(N, kind, sd)
        pc.case_route(N, kind, sd)
        pc.case_kpos(N, kind, sd)
        pc.case_zero_entries(N, kind, sd)
        pc.case_coo_ones(N, kind, sd)
    for me in range(N):
        pc.eager_shares(N, me)


def test_inputs_are_the_same_on_every_rank():
    """seeded: two builds of a case are identical (every rank generates its own copy)"""
    a, b = pc.case_transpose(3, "ragged", 1), pc.case_transpose(3, "ragged", 1)
    for (_, A, rs, cs), (_, B, rs2, cs2) in zip(a, b):
        assert refops.same(A, B) and np.array_equal(rs, rs2) and np.array_equal(cs, cs2)


@pytest.mark.parametrize("N,kind", pc.LAUNCHES, ids=IDS)
def test_transpose_model(N, kind):
    """rank q transposes its rows; the owner concatenates the pieces in rank order: the stable
    whole-matrix transpose (ascending global row within a column)"""
    for name, A, rs, cs in pc.case_transpose(N, kind, 0):
        assert pc.diff_csr(pc.model_transpose(A, rs, cs), refops.transpose(A)) is None, name


@pytest.mark.parametrize("N,kind", pc.LAUNCHES, ids=IDS)
def test_halo_model(N, kind):
    """the local rows of A times the assembled halo view of B are the local rows of A * B, and
    the view holds exactly B's own and referenced rows"""
    for name, A, B, rs, ms, ks in pc.case_spgemm(N, kind, 0):
        want = refops.spgemm(A, B)
        for me in range(N):
            L = pc.block(A, rs[me], rs[me + 1])
            E = pc.model_halo(B, ms, me, L.col)
            assert pc.diff_csr(refops.spgemm(L, E), pc.block(want, rs[me], rs[me + 1])) is None, (name, me)
            used = set(L.col.tolist()) | set(range(ms[me], ms[me + 1]))
            for i in range(B.rn):
                ln = E.row_off[i + 1] - E.row_off[i]
                assert ln == (B.row_off[i + 1] - B.row_off[i] if i in used else 0)
        if name == "block_diag":
            for me in range(N):
                assert all(ms[me] <= c < ms[me + 1] for c in pc.block(A, rs[me], rs[me + 1]).col)


@pytest.mark.parametrize("N,kind", pc.LAUNCHES, ids=IDS)
def test_route_and_list_models(N, kind):
    for name, I, J, V, parts, s in pc.case_route(N, kind, 0):
        got = pc.model_route(I, J, V, parts, s)
        assert sum(len(g[0]) for g in got) == len(I)
        own = np.array([pc.owner_of(s, i) for i in I])
        for p in range(N):                 # a stable partition of the concatenated entries
            sel = np.nonzero(own == p)[0]
            assert np.array_equal(got[p][0], I[sel]) and np.array_equal(got[p][1], J[sel])
            assert np.array_equal(pc.bits(got[p][2]), pc.bits(V[sel]))
    finals = []
    for me in range(N):                    # after a sync every rank holds the owners' values
        name, s, lst, z0, want = pc.case_list_sync(N, kind, 0, me)[0]
        assert all(want[i] == z0[i] for i in range(len(z0)) if i not in set(lst.tolist()))
        assert all(z0[i] == -1000.0 - me for i in range(len(z0)) if not s[me] <= i < s[me + 1])
        finals.append(want[np.sort(lst)])
    assert all(np.array_equal(f, finals[0]) for f in finals)


def test_reference_restatements():
    """the small host references of part_cases against numpy on a dense copy"""
    rng = np.random.default_rng(5)
    A = refops.rand_csr(rng, 40, 30, 0.2)
    D = np.zeros((40, 30))
    for i, (c, v) in enumerate(pc.to_rows(A)):
        D[i, c] = v
    vr, vc = (rng.random(40) < 0.5), (rng.random(30) < 0.5)
    S = pc.ref_sub_mat(A, vr.astype(np.uint8), vc.astype(np.uint8))
    Sd = np.zeros((S.rn, S.cn))
    for i, (c, v) in enumerate(pc.to_rows(S)):
        Sd[i, c] = v
    assert np.array_equal(Sd, D[vr][:, vc])
    assert np.array_equal(pc.ref_induced(np.array([0, 10, 40]), vr.astype(np.uint8)), [0, vr[:10].sum(), vr.sum()])
    sq = pc.from_rows(pc.to_rows(refops.rand_csr(rng, 30, 30, 0.3, minrow=30)), 30)
    assert np.array_equal(pc.ref_diag(sq), [v[c.index(i)] for i, (c, v) in enumerate(pc.to_rows(sq))])
    k = pc.ref_kpos(A)
    T = refops.transpose(A)
    for i in range(A.rn):
        for e in range(A.row_off[i], A.row_off[i + 1]):
            assert T.col[T.row_off[A.col[e]] + int(k[e])] == i
    sl = pc.eager_expect_slots(pc.eager_shares(4, 0))
    assert [s for s, _ in sl][:2] == [4096, 4096] and sl[2][1] and not sl[1][1] and sl[5][1]
    assert sl[6][0] == 1 << 20 and not sl[6][1]
    assert all(sec == (max(c) > 8) for c, (_, sec) in zip(pc.eager_shares(4, 0), pc.eager_expect_slots(
        pc.eager_shares(4, 0), 8)))
