"""One rank of the partitioned-solve tests (tests/test_gpu_part_solve.py; DESIGN.md "Solve",
the partitioned part).  Launched like tests/part_worker.py: N processes on the same GPU over
the host transport with RANK / WORLD_SIZE / MASTER_PORT set and the collective guard on.
PS_WHAT selects the work of the launch:

  cycle  one partitioned setup of PS_CASE, then amgd_solve_device in every mode in this
         process -- {halo, allgather} x replication {0, default, everything, PS_REPL extra
         limits} x {fused default, cooperative kernels on, composed}, with and without the
         mean -- against refsolve.vcycle on the hierarchy exported by the same run
  halo   the halo exchange on its own, every partition kind of tests/part_cases.py, 3 seeds
  crs    crs_setup + crs_solve (PS_CASE crs4 / amgdmp) in the partitioned and the replicated
         setup mode against refsolve_part.crs_solve_ranks

Prints one JSON line; exit code 0 = every comparison passed."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import omp_amg_amd as oa  # noqa: E402
from omp_amg_amd import abi, problems, shard  # noqa: E402
import part_cases as pc  # noqa: E402
import refsolve  # noqa: E402
import refsolve_part  # noqa: E402

POISON = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
KERNELS = {"fused": (-1, -1), "coop": (1, 1), "composed": (0, -1)}       # (vc_fused, vc_coop)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def coo(case):
    if case.startswith("gold:"):
        z = np.load(os.path.join(HERE, "golden", case[5:] + ".npz"))
        return z["in_Ai"], z["in_Aj"], z["in_Av"]
    if case.startswith("p7:"):
        return problems.poisson3d(int(case[3:]))
    raise ValueError(case)


def run_cycle(rank, size, out):
    L = oa.lib()
    Ai, Aj, Av = coo(os.environ["PS_CASE"])
    Ai, Aj, Av = np.asarray(Ai, np.int64), np.asarray(Aj, np.int64), np.asarray(Av)
    nz = len(Av)
    k0, k1 = rank * nz // size, (rank + 1) * nz // size
    ds = oa.DeviceSetup(Ai[k0:k1], Aj[k0:k1], Av[k0:k1])
    ds.run()
    h = ds.export()
    n0 = int(h.levels[0].n)
    r0, r1 = ds.rows()
    b = np.random.default_rng(11).standard_normal(n0)
    ref = {f: refsolve.vcycle(h, b, remove_mean=f) for f in (False, True)}
    # replication limits: 0 (the bottom level only), the default, everything; PS_REPL=level1:
    # level 1's slice size (level 1 replicated) and one less (level 1 distributed)
    n1 = n0 - int(np.count_nonzero(np.asarray(h.levels[0].F))) if h.nlevels > 1 else 0
    repls = [0, -1, 1 << 40] + ([n1, n1 - 1] if os.environ.get("PS_REPL") == "level1" else [])
    bad, stats = [], {}
    for repl in repls:
        oa.vc_repl(repl)
        for halo in (1, 0):
            oa.vc_halo(halo)
            for kname, (fused, coop) in KERNELS.items():
                oa.vc_fused(fused)
                oa.vc_coop(coop)
                for mean in (False, True):
                    tag = f"repl={repl} halo={halo} {kname} mean={int(mean)}"
                    oa.route_stats()
                    x1 = ds.solve(b, remove_mean=mean, partitioned=True)
                    st = oa.solve_comm_stats()
                    rs = oa.route_stats()
                    if not np.array_equal(bits(ds.b_after), bits(b)):
                        bad.append(tag + ": db changed")
                    if not np.array_equal(bits(x1[r0:r1]), bits(ref[mean][r0:r1])):
                        bad.append(tag + ": own rows differ")
                    if size > 1 and not (np.all(np.isnan(x1[:r0])) and np.all(np.isnan(x1[r1:]))):
                        bad.append(tag + ": rows of another rank written")
                    # the second call, completing x on every rank (flag bit 1): every row
                    x2 = ds.solve(b, remove_mean=mean, complete=True, partitioned=True)
                    if not np.array_equal(bits(x2), bits(ref[mean])):
                        bad.append(tag + ": completed x differs")
                    # route counters match the forced mode
                    if rs["vc_halo" if not halo else "vc_allg"] != 0:
                        bad.append(tag + f": the other exchange mode ran {rs}")
                    if repl == 1 << 40 and (rs["vc_halo"] or rs["vc_allg"] or (h.nlevels > 1 and not rs["vc_repl"])):
                        bad.append(tag + f": everything replicated, yet {rs}")
                    if size > 1 and repl == 0:
                        # at N > 1 with replication 0 every rank makes at least one collective per cycle
                        if st["collectives"] < 1:
                            bad.append(tag + ": no collective")
                        if h.nlevels > 2 and not rs["vc_halo" if halo else "vc_allg"]:
                            bad.append(tag + f": the forced exchange mode did not run {rs}")
                    stats[tag] = [st["collectives"], st["bytes"]]
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_halo, oa.vc_repl):
        f(-1)
    ds.close()
    out.update(levels=h.nlevels, n0=n0, rows=[r0, r1], stats=stats)
    return bad


def run_halo(rank, size, out):
    bad = []
    for kind, seed in [(k, s) for k in pc.KINDS for s in range(3)]:
        rng = np.random.default_rng(200 + seed)
        rn, cn = 301, 257
        M = pc.with_row_lengths(rng, rn, cn, rng.integers(0, 9, rn))
        rs, vs = pc.split(kind, rn, size, seed), pc.split(kind, cn, size, seed + 7)
        truth = rng.standard_normal(cn)
        v = np.full(cn, POISON)
        v[vs[rank]:vs[rank + 1]] = truth[vs[rank]:vs[rank + 1]]
        got = oa.test_vc_halo_xch(M, rs, vs, v)
        cols = M.col[M.row_off[rs[rank]]:M.row_off[rs[rank + 1]]]
        lists = refsolve_part.halo_lists(cols, vs, rank)
        want = v.copy()                      # own entries: truth; referenced: truth; the rest: poison
        for idx in lists.values():
            want[idx] = truth[idx]
        d = pc.diff_vec(got, want)
        if d:
            bad.append(f"{kind} seed {seed}: {d}")
    return bad


CRS_A = np.array([2, -1, -1, 0, -1, 2, 0, -1, -1, 0, 2, -1, 0, -1, -1, 2], dtype=np.float64)


def crs_case(case, size):
    """per rank: (n, ids, Ai, Aj, Av, b, x0), global (n0, null_space).  Every rank holds a
    block of rows of the matrix with scrambled ids; its local dofs are the ids its entries touch
    (so dofs are shared between ranks), two id-0 dofs and one dof twice"""
    if case == "crs4":
        I, J, V, null = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4), CRS_A, 1
    else:
        z = np.load(os.path.join(HERE, "golden", "amgdmp.npz"))
        I, J, V, null = z["in_Ai"].astype(np.int64), z["in_Aj"].astype(np.int64), z["in_Av"], 1
    keep = V != 0
    I, J, V = I[keep], J[keep], V[keep]
    n0 = int(max(I.max(), J.max())) + 1
    rng = np.random.default_rng(7)
    perm = rng.permutation(n0)                 # row i of the matrix has global id perm[i] + 1
    ranks = []
    for r in range(size):
        lo, hi = r * n0 // size, (r + 1) * n0 // size
        sel = (I >= lo) & (I < hi)
        dofs = np.unique(np.concatenate([I[sel], J[sel]]))
        dofs = dofs[rng.permutation(len(dofs))]
        loc = {int(g): k for k, g in enumerate(dofs)}
        n = len(dofs) + 3
        ids = np.concatenate([perm[dofs] + 1, [0, 0, perm[dofs[0]] + 1]])
        Ai = np.array([loc[int(g)] for g in I[sel]], dtype=np.int64)
        Aj = np.array([loc[int(g)] for g in J[sel]], dtype=np.int64)
        ranks.append((n, ids, Ai, Aj, V[sel], rng.standard_normal(n), np.full(n, 42.0)))
    return ranks, n0, null


def run_crs(rank, size, out):
    L = oa.lib()
    ranks, n0, null = crs_case(os.environ["PS_CASE"], size)
    n, ids, Ai, Aj, Av, b, x0 = ranks[rank]
    bad = []
    for mode in ("partitioned", "replicated"):
        L.amgd_comm_set_partitioned(1 if mode == "partitioned" else 0)
        hd = abi.crs_setup(L, n, ids, Ai, Aj, Av, null_space=null, rank=rank, np_=size)
        if hd is None:
            return [mode + ": crs_setup returned NULL"]
        h = abi.crs_export(L, hd)
        x = abi.crs_solve(L, hd, b, x0=x0)
        if not np.array_equal(bits(abi.crs_solve.b_after), bits(b)):
            bad.append(mode + ": b modified")
        x2 = abi.crs_solve(L, hd, b, x0=x0)
        L.crs_free(hd)
        want = refsolve_part.crs_solve_ranks(h, [q[1] for q in ranks], [q[5] for q in ranks], null,
                                             x0=[q[6] for q in ranks])[rank]
        for name, g in (("x", x), ("second x", x2)):
            d = pc.diff_vec(g, want)
            if d:
                bad.append(f"{mode}: {name} {d}")
        if not (x[n - 3] == 42.0 and x[n - 2] == 42.0 and bits(x[n - 1:])[0] == bits(x[:1])[0]):
            bad.append(mode + ": id-0 dofs or the repeated dof")
    return bad


def main():
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    oa.init(0)
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    before = L.amgd_test_pool_inuse()
    shard.init_host(rank, size)
    what = os.environ["PS_WHAT"]
    out = {"rank": rank, "size": size, "what": what}
    if what != "crs":
        L.amgd_comm_set_partitioned(1)
    bad = {"cycle": run_cycle, "halo": run_halo, "crs": run_crs}[what](rank, size, out)
    # after amgd_hier_free / crs_free nothing of the solve stays on the device
    out["leak_bytes"] = int(L.amgd_test_pool_inuse()) - int(before)
    out["bad"] = bad[:12]
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not bad and out["leak_bytes"] == 0 else 1)


if __name__ == "__main__":
    main()
