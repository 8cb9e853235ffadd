"""One rank of the row-partitioned primitive tests (tests/test_gpu_part_prims.py).

Launched like part_worker.py (gloo group, host transport, the collective guard on).  One
launch runs every pm_* operation of amgd_part.h for one (WORLD_SIZE, PART_CASE = partition
kind) on the inputs of tests/part_cases.py, each through amgd_test_pm: the rank uploads its
rows of the whole operands, makes ONE pm_* call and compares what comes back, bit for bit,
with the host restatement of the one-GPU operation on the whole matrix (tests/refops.py).

Every rank makes the same sequence of calls whatever it finds: a comparison only records a
failure, it never decides whether a collective runs.  Prints one JSON line with every failing
(op, case) and its first differing row / entry; exit code 1 if any case failed or device
bytes stay held."""
import ctypes as C
import json
import math
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import omp_amg_amd as oa  # noqa: E402
from omp_amg_amd import shard  # noqa: E402
import part_cases as pc  # noqa: E402
import refops  # noqa: E402

SEEDS = (0, 1, 2)
BAD = []
NCHECK = [0]


def check(op, case, fn):
    """fn() -> None or a description of the first difference; exceptions are failures too"""
    NCHECK[0] += 1
    try:
        with np.errstate(all="ignore"):
            d = fn()
    except Exception:  # noqa: BLE001 -- a broken comparison must not change the call sequence
        d = "exception: " + traceback.format_exc(limit=3)[-400:]
    if d is not None:
        BAD.append({"op": op, "case": case, "diff": d})


def rows(E, s, me):
    return pc.block(E, int(s[me]), int(s[me + 1]))


def sentinel(n, me):
    return np.full(n, -7000.0 - me)


def run_induced(N, kind, me):
    for sd in SEEDS:
        for name, s, mask in pc.case_induced(N, kind, sd):
            r = oa.test_pm("induced", ars=s, f=mask)
            check("apart_induced", f"{name}/s{sd}",
                  lambda: None if np.array_equal(r["so_r"], pc.ref_induced(s, mask)) else
                  f"{r['so_r'].tolist()} != {pc.ref_induced(s, mask).tolist()}")


def run_transpose(N, kind, me):
    for sd in SEEDS:
        for name, A, rs, cs in pc.case_transpose(N, kind, sd):
            r = oa.test_pm("transpose", A=A, ars=rs, acs=cs)
            check("pm_transpose", f"{name}/s{sd}", lambda: pc.diff_csr(r["X"], rows(refops.transpose(A), cs, me)))


def run_spgemm(N, kind, me):
    for sd in SEEDS:
        for name, A, B, rs, ms, ks in pc.case_spgemm(N, kind, sd):
            tag = f"{name}/s{sd}"
            Lc = rows(A, rs, me).col
            for nocol in (False, True):
                r = oa.test_pm("halo", A=A, B=B, ars=rs, acs=ms, brs=ms, bcs=ks, b_nocol=nocol)
                check("pm_halo_rows" + ("(values-only)" if nocol else ""), tag,
                      lambda: ("col present" if nocol and r["X"].col is not None else
                               pc.diff_csr(r["X"], pc.model_halo(B, ms, me, Lc), cols=not nocol)))
            r = oa.test_pm("spgemm", A=A, B=B, ars=rs, acs=ms, brs=ms, bcs=ks, iarg=0)
            check("pm_spgemm", tag, lambda: pc.diff_csr(r["X"], rows(refops.spgemm(A, B), rs, me)))
            Ap, Bp = pc.positive(A), pc.positive(B)
            r = oa.test_pm("spgemm", A=Ap, B=Bp, ars=rs, acs=ms, brs=ms, bcs=ks, iarg=1)
            check("pm_spgemm(pattern)", tag,
                  lambda: pc.diff_csr(r["X"], rows(refops.spgemm(Ap, Bp), rs, me), vals=False))


def run_sub_mat(N, kind, me):
    for sd in SEEDS:
        for name, A, rs, cs, vr, vc in pc.case_sub_mat(N, kind, sd):
            r = oa.test_pm("sub_mat", A=A, ars=rs, acs=cs, vr=vr, vc=vc)

            def cmp():
                wr, wc = pc.ref_induced(rs, vr), pc.ref_induced(cs, vc)
                if not (np.array_equal(r["so_r"], wr) and np.array_equal(r["so_c"], wc)):
                    return f"induced splits {r['so_r'].tolist()} {r['so_c'].tolist()} != {wr.tolist()} {wc.tolist()}"
                return pc.diff_csr(r["X"], rows(pc.ref_sub_mat(A, vr, vc), wr, me))
            check("pm_sub_mat", f"{name}/s{sd}", cmp)


def run_vec(N, kind, me):
    for sd in SEEDS:
        A, s = pc.case_vec(N, kind, sd)
        n = A.rn
        rng = np.random.default_rng(sd + 7)
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        f = (rng.random(n) < 0.7).astype(np.uint8)
        tag = f"s{sd}"
        z0 = sentinel(n, me)
        for nm, kw, want in (
                ("y,f", dict(alpha=0.75, y=y, beta=-1.25, f=f), lambda: pc.ref_spmv_f(A, x, 0.75, y, -1.25, f)),
                ("plain", dict(alpha=0.0, beta=1.0), lambda: refops.spmv(A, x))):
            r = oa.test_pm("spmv", A=A, ars=s, acs=s, x=x, z=z0, **kw)
            check(f"pm_spmv({nm})", tag, lambda: pc.diff_vec(r["z"], want()))
        for op, want in (("spmvt", lambda: refops.spmv(A, x)), ("colsum", lambda: pc.rowsums(A)),
                         ("diag", lambda: pc.ref_diag(A)), ("rowsum_sq_inv", lambda: pc.ref_rowsum_sq_inv(A))):
            r = oa.test_pm(op, A=A, ars=s, acs=s, x=x, z=z0)
            check("pm_" + op, tag, lambda: pc.diff_vec(r["z"], want()))
        Dl, Dr = rng.standard_normal(n), rng.standard_normal(n)
        for op in (0, 1):
            r = oa.test_pm("diag_op", A=A, ars=s, acs=s, x=Dl, iarg=op)
            check(f"pm_diag_op({op})", tag, lambda: pc.diff_csr(r["X"], rows(pc.ref_diag_op(A, Dl, None, op), s, me)))
        for op in (4, 5, 6, 7):
            r = oa.test_pm("diag_op2", A=A, ars=s, acs=s, x=Dl, y=Dr, iarg=op)
            check(f"pm_diag_op2({op})", tag, lambda: pc.diff_csr(r["X"], rows(pc.ref_diag_op(A, Dl, Dr, op), s, me)))
        # ||A - I||_F^2: exactly 0 for a partitioned identity, else within nnz * 2^-52 (relative)
        r = oa.test_pm("fro", A=A, ars=s, acs=s)

        def cmp_fro():
            sq = []
            for i, (c, v) in enumerate(pc.to_rows(A)):
                done = False
                for j, a in zip(c, v):
                    if j == i and not done:
                        a, done = a - 1.0, True
                    sq.append(a * a)
            want = math.fsum(sq)
            ok = abs(r["scalar"] - want) <= len(sq) * 2.0 ** -52 * want
            return None if ok else f"{r['scalar']!r} vs fsum {want!r} (nnz {len(sq)})"
        check("pm_fro_minus_eye", tag, cmp_fro)
        Id = pc.from_rows([([i], [1.0]) for i in range(n)], n)
        r = oa.test_pm("fro", A=Id, ars=s, acs=s)
        check("pm_fro_minus_eye", f"identity/{tag}",
              lambda: None if r["scalar"] == 0.0 and not math.copysign(1, r["scalar"]) < 0 else repr(r["scalar"]))


def run_rowops(N, kind, me):
    for sd in SEEDS:
        A, B, rs, cs, mask = pc.case_rowops(N, kind, sd)
        tag = f"s{sd}"
        for al, be in ((1.0, -1.0), (0.5, 2.0)):
            r = oa.test_pm("mpm", A=A, B=B, ars=rs, acs=cs, brs=rs, bcs=cs, alpha=al, beta=be)
            check(f"pm_mpm({al},{be})", tag, lambda: pc.diff_csr(r["X"], rows(refops.mpm(al, A, be, B), rs, me)))
        r = oa.test_pm("mxmpoint", A=A, B=B, ars=rs, acs=cs, brs=rs, bcs=cs)
        check("pm_mxmpoint", tag, lambda: pc.diff_csr(r["X"], rows(refops.mxmpoint(A, B), rs, me)))
        r = oa.test_pm("drop_zeros", A=A, ars=rs, acs=cs)
        check("pm_drop_zeros", tag, lambda: pc.diff_csr(r["X"], rows(pc.ref_drop_zeros(A), rs, me)))
        r = oa.test_pm("rows_masked", A=A, ars=rs, acs=cs, f=mask)
        check("pm_rows_masked", tag, lambda: pc.diff_csr(r["X"], rows(pc.ref_rows_masked(A, mask), rs, me)))
        for nocol in (False, True):
            r = oa.test_pm("gather_full", A=B, ars=rs, acs=cs, a_nocol=nocol)
            check("pm_gather_full" + ("(values-only)" if nocol else ""), tag,
                  lambda: ("col present" if nocol and r["X"].col is not None else
                           pc.diff_csr(r["X"], B, cols=not nocol)))
        r = oa.test_pm("gather_pattern", A=B, ars=rs, acs=cs)
        check("pm_gather_pattern", tag,
              lambda: "values present" if r["X"].a is not None else pc.diff_csr(r["X"], B, vals=False))


def run_lists(N, kind, me):
    for sd in SEEDS:
        cs = pc.case_list_sync(N, kind, sd, me)
        for name, s, lst, z0, want in cs:
            r = oa.test_pm("list_sync", ars=s, li=lst, z=z0)
            check("pm_list_sync", f"{name}/s{sd}", lambda: pc.diff_vec(r["z"], want))
        (_, s1, l1, z1, w1), (_, s2, l2, z2, w2) = cs[0], cs[3]       # two spaces, two partitions
        r = oa.test_pm("list_sync2", ars=s1, brs=s2, li=l1, lj=l2, z=z1, z2=z2)
        check("pm_list_sync_n", f"s{sd}", lambda: pc.diff_vec(r["z"], w1) or pc.diff_vec(r["z2"], w2))
        (A, sa), (B, sb), la, lb = pc.case_list_rowsum(N, kind, sd)
        la = np.random.default_rng(sd + 31 * me).permutation(la)
        lb = np.random.default_rng(sd + 31 * me + 5).permutation(lb)
        za, zb = sentinel(A.rn, me), sentinel(B.rn, me)

        def want(M, lst, z0):
            w = z0.copy()
            w[lst] = pc.rowsums(M)[lst]
            return w
        for M, s, lst, z0, nm in ((A, sa, la, za, "A"), (B, sb, lb, zb, "B")):
            r = oa.test_pm("list_rowsum", A=M, ars=s, acs=pc.split("even", M.cn, N), li=lst, z=z0)
            check("pm_list_rowsum", f"{nm}/s{sd}", lambda: pc.diff_vec(r["z"], want(M, lst, z0)))
        ce = pc.split("even", A.cn, N)
        r = oa.test_pm("list_rowsum2", A=A, B=B, ars=sa, acs=ce, brs=sb, bcs=ce, li=la, lj=lb, z=za, z2=zb)
        check("pm_list_rowsum2", f"s{sd}",
              lambda: pc.diff_vec(r["z"], want(A, la, za)) or pc.diff_vec(r["z2"], want(B, lb, zb)))


def eager_stats():
    ps = (C.c_uint64 * 4)()
    oa.lib().amgd_test_part_stats(ps)
    return int(ps[2]), int(ps[3])


def run_eager(N, kind, me, forced):
    calls = pc.eager_shares(N, me)
    seqs = [(0, calls), (0, [[5000 + p for p in range(N)]]), (1, [[5000 + p for p in range(N)]])]
    big = max(x for c in calls for x in c)
    k = 0
    for part, (state, cl) in enumerate(seqs):
        if part == 1:
            oa.lib().amgd_test_pm_eager_new_setup()      # every state back to the default slot
        exp = pc.eager_expect_slots(cl, forced)
        for c, (slot, second) in zip(cl, exp):
            mine = pc.eager_payload(k, me, c[me])
            c0, s0 = eager_stats()
            out, ln, us, tot, slot_after = oa.test_pm_eager(state, mine, 100 * k + me, N, sum(c) if sum(c) else 8)
            c1, s1 = eager_stats()

            def cmp(k=k, c=c, second=second):
                if ln.tolist() != c or tot != sum(c) or us.tolist() != [100 * k + p for p in range(N)]:
                    return f"len {ln.tolist()} users {us.tolist()} total {tot}"
                want = b"".join(pc.eager_payload(k, p, c[p]) for p in range(N))
                if out != want:
                    i = next(i for i in range(len(want)) if out[i] != want[i])
                    return f"payload differs first at byte {i} of {len(want)}"
                mx = max(c)
                ns = min(max(mx + mx // 4, 4096), 1 << 20)
                if slot_after != ns:
                    return f"slot after the call {slot_after} != {ns}"
                if (c1 - c0, s1 - s0) != (1, int(second)):
                    return f"second rounds counted {s1 - s0}, expected {int(second)} (slot {slot})"
                return None
            check("pm_allgather_dyn", f"part{part}/call{k}/shares{[x if x < big else '3MB+5' for x in c]}", cmp)
            k += 1


def run_route(N, kind, me):
    for sd in SEEDS:
        for name, I, J, V, parts, s in pc.case_route(N, kind, sd):
            k0, k1 = parts[me]
            r = oa.test_pm("route_coo", ars=s, li=I[k0:k1], lj=J[k0:k1], x=V[k0:k1])

            def cmp():
                wi, wj, wv = pc.model_route(I, J, V, parts, s)[me]
                if not (np.array_equal(r["rows"], wi) and np.array_equal(r["X"].col, wj)):
                    return f"{len(r['rows'])} entries, expected {len(wi)}; or their order differs"
                return pc.diff_vec(r["X"].a, wv)
            check("pm_route_coo", f"{name}/s{sd}", cmp)


def run_misc(N, kind, me):
    for sd in SEEDS:
        A, rs, cs = pc.case_kpos(N, kind, sd)
        r = oa.test_pm("kpos", A=A, ars=rs, acs=cs)
        check("pm_kpos", f"s{sd}", lambda: pc.diff_csr(
            r["X"], rows(pc.Csr(A.rn, A.cn, A.row_off, A.col, pc.ref_kpos(A)), rs, me)))
        A, rs, cs, ri, cj = pc.case_zero_entries(N, kind, sd)
        r = oa.test_pm("zero_entries", A=A, ars=rs, acs=cs, li=ri, lj=cj)
        check("pm_zero_entries", f"s{sd}", lambda: pc.diff_csr(r["X"], rows(pc.ref_zero_entries(A, ri, cj), rs, me)))
        rs, cs, ri, cj = pc.case_coo_ones(N, kind, sd)
        r = oa.test_pm("coo_ones", ars=rs, acs=cs, li=ri, lj=cj)

        def cmp():
            o = np.lexsort((cj, ri))                      # stable by (i, j); repeats kept
            ro = np.concatenate([[0], np.cumsum(np.bincount(ri, minlength=int(rs[-1])))])
            E = pc.Csr(int(rs[-1]), int(cs[-1]), ro, cj[o], np.ones(len(ri)))
            return pc.diff_csr(r["X"], rows(E, rs, me))
        check("pm_coo_ones", f"s{sd}", cmp)


def main():
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    kind = os.environ["PART_CASE"]
    dist.init_process_group("gloo", rank=rank, world_size=size)
    oa.init(0)
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    before = int(L.amgd_test_pool_inuse())
    shard.init_host(rank, size)
    L.amgd_comm_set_partitioned(1)
    forced = int(os.environ.get("PART_EAGER_SLOT", "0"))
    L.amgd_test_part_force.argtypes = [C.c_int, C.c_int64]
    L.amgd_test_part_force(0, forced)
    shard.stats(reset=True)
    groups = os.environ.get("PART_GROUPS", "")
    for name, fn in (("induced", run_induced), ("transpose", run_transpose), ("spgemm", run_spgemm),
                     ("sub_mat", run_sub_mat), ("vec", run_vec), ("rowops", run_rowops), ("lists", run_lists),
                     ("route", run_route), ("misc", run_misc)):
        if not groups or name in groups.split(","):
            fn(size, kind, rank)
    if not groups or "eager" in groups.split(","):
        run_eager(size, kind, rank, forced)
    st = shard.stats()
    out = {"rank": rank, "kind": kind, "size": size, "checks": NCHECK[0], "bad": BAD, "calls": st["calls"],
           "leak_bytes": int(L.amgd_test_pool_inuse()) - before}
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not BAD and NCHECK[0] > 0 and st["calls"] > 0 and out["leak_bytes"] == 0 else 1)


if __name__ == "__main__":
    main()
