"""One rank of the partitioned Krylov tests (tests/test_gpu_part_krylov.py; DESIGN.md "Krylov on
the row-partitioned hierarchy").  Launched like tests/part_solve_worker.py: N processes on the
same GPU over the host transport with RANK / WORLD_SIZE / MASTER_PORT set and the collective
guard on.  PK_WHAT selects the work of the launch:

  solve    one partitioned setup of PK_CASE, then amgd_krylov_device with flag bit 2: the ordered
           path against refkrylov.fgmres on the hierarchy the same run exported (restart 30 and
           5 in halo and allgather mode with replication 0 and default; a guess, maxit 4, bit 3,
           a repeat), the fused path's criteria, the collective count
           against the documented formula, the workspace's size
  combine  the rank-order combine of the multi-dot and of the update's norm on their own
  product  the level-0 product with its halo exchange on its own
  crs      crs_setup + amgd_crs_krylov (PK_CASE crs4 / amgdmp) in the partitioned and the
           replicated setup mode against the rank-aware restatement

Prints one JSON line; exit code 0 = every comparison passed."""
import ctypes as C
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import omp_amg_amd as oa  # noqa: E402
from omp_amg_amd import abi, shard  # noqa: E402
import part_cases as pc  # noqa: E402
import part_solve_worker as psw  # noqa: E402
import refkrylov  # noqa: E402
import refsolve  # noqa: E402
import refsolve_part  # noqa: E402

RTOL, MAXIT = 1e-10, 30
POISON = psw.POISON
bits = psw.bits
INFO_KEYS = ("rc", "its", "restarts", "cycles", "converged", "bnorm", "r0", "resid")


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def info_diff(info, want):
    """the fields of amgd_krylov_info and rc against the restatement's, floats bit for bit"""
    return [k for k in INFO_KEYS if not same(np.float64(info[k]), np.float64(want[k]))]


def count_formula(its, restarts, cyc, px, guess, complete):
    """collectives of a fused partitioned call with its > 0 (omp_amg_amd.h, amgd_krylov_comm_stats)"""
    return 1 + guess * (px + 1) + its * (cyc + px + 3) + (restarts + 1) * (px + 1) + (1 if complete else 0)


def all_same(obj):
    """the object is equal on every rank"""
    got = [None] * dist.get_world_size()
    dist.all_gather_object(got, obj)
    return all(g == got[0] for g in got)


def run_solve(rank, size, out):
    L = oa.lib()
    Ai, Aj, Av = psw.coo(os.environ["PK_CASE"])
    Ai, Aj, Av = np.asarray(Ai, np.int64), np.asarray(Aj, np.int64), np.asarray(Av)
    nz = len(Av)
    k0, k1 = rank * nz // size, (rank + 1) * nz // size
    ds = oa.DeviceSetup(Ai[k0:k1], Aj[k0:k1], Av[k0:k1])
    ds.run()
    h = ds.export()
    A = h.levels[0].A
    n0 = int(h.levels[0].n)
    null = bool(h.nullspace)
    r0, r1 = ds.rows()
    xs = np.random.default_rng(5).standard_normal(n0)
    if null:
        xs = xs - xs.mean()
    b = refsolve.csr_matvec(A, xs)                       # b = A x*, as test_gpu_krylov.problem
    bad = []
    # px: does a rank's row block of A read an entry another rank owns (the halo list's global count)
    rows = [None] * size
    dist.all_gather_object(rows, (r0, r1))
    ro, col = np.asarray(A.row_off), np.asarray(A.col)
    foreign = any(np.any((col[ro[a]:ro[c]] < a) | (col[ro[a]:ro[c]] >= c)) for a, c in rows)

    def check_ordered(tag, want, x0=None, complete=False, **kw):
        x, info, hist = ds.krylov(b, rtol=RTOL, ordered=True, partitioned=True, x0=x0, complete=complete, check=False, **kw)
        if not same(ds.b_after, b):
            bad.append(tag + ": db changed")
        if info_diff(info, want):
            bad.append(tag + f": info differs in {info_diff(info, want)}: {info}")
            return None
        if not same(hist, np.array(want["hist"])):
            bad.append(tag + ": hist differs")
        if not same(x[r0:r1], want["x"][r0:r1]):
            bad.append(tag + ": own rows differ")
        rest = np.concatenate([x[:r0], x[r1:]])
        if complete:
            if not same(x, want["x"]):
                bad.append(tag + ": completed x differs")
        elif size > 1:
            other = np.full(n0, np.nan) if x0 is None else x0
            if not np.array_equal(bits(rest), bits(np.concatenate([other[:r0], other[r1:]]))):
                bad.append(tag + ": rows of another rank written")
        return x, info, hist

    # the plan first (so that the first Krylov call's pool growth is the workspace), and cyc
    ds.solve(b, remove_mean=null, partitioned=True)
    refs = {m: refkrylov.fgmres(h, b, rtol=RTOL, restart=m, maxit=MAXIT) for m in (30, 5)}
    L.amgd_test_pool_inuse.restype = C.c_uint64
    before = int(L.amgd_test_pool_inuse())
    first = ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT, partitioned=True, check=False)
    out["ws_growth"] = int(L.amgd_test_pool_inuse()) - before
    out["ws_one_gpu"] = (2 * 30 + 4) * n0 * 8
    # ---- 1. ordered, bit for bit, in every exchange mode
    for restart in (30, 5):
        for halo in (1, 0):
            for repl in (0, -1):
                oa.vc_halo(halo)
                oa.vc_repl(repl)
                check_ordered(f"ordered m={restart} halo={halo} repl={repl}", refs[restart], restart=restart, maxit=MAXIT)
    oa.vc_halo(-1)
    oa.vc_repl(-1)
    x0 = refsolve.vcycle(h, b, remove_mean=null)
    check_ordered("ordered guess", refkrylov.fgmres(h, b, rtol=RTOL, restart=30, maxit=MAXIT, x0=x0), x0=x0,
                  restart=30, maxit=MAXIT)
    want4 = refkrylov.fgmres(h, b, rtol=RTOL, restart=30, maxit=4)
    if want4["rc"] != 1:
        bad.append("maxit 4: the restatement converged, the case lost its property")
    check_ordered("ordered maxit 4", want4, restart=30, maxit=4)
    a1 = check_ordered("ordered complete", refs[30], complete=True, restart=30, maxit=MAXIT)
    a2 = check_ordered("ordered complete again", refs[30], complete=True, restart=30, maxit=MAXIT)
    if a1 and a2 and not (same(a1[0], a2[0]) and same(a1[2], a2[2]) and a1[1] == a2[1]):
        bad.append("ordered: the second call differs")
    # ---- 2. fused: the criteria of test_fused_path_converges_and_repeats, the counts
    stats = {}
    bn = float(np.linalg.norm(b))
    for halo in (1, 0):
        oa.vc_halo(halo)
        ds.solve(b, remove_mean=null, partitioned=True)
        cyc = oa.solve_comm_stats()["collectives"]
        px = 0 if size == 1 else (1 if (not halo or foreign) else 0)
        for restart in ((30, 5) if halo else (30,)):         # allgather mode: the count and the criteria once
            tag = f"fused m={restart} halo={halo}"
            oa.route_stats()
            x, info, hist = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, partitioned=True, complete=True, check=False)
            rs = oa.route_stats()
            st = oa.krylov_comm_stats()
            res = float(np.linalg.norm(b - refsolve.csr_matvec(A, x))) / bn if info["rc"] >= 0 else float("nan")
            print(tag, "its", info["its"], "ordered", refs[restart]["its"], "relative residual", res, flush=True)
            if info["rc"] != 0 or info["converged"] != 1:
                bad.append(tag + f": rc {info}")
                continue
            if abs(info["its"] - refs[restart]["its"]) > 1:
                bad.append(tag + f": its {info['its']} against the ordered {refs[restart]['its']}")
            if not res <= RTOL * (1 + 1e-3):
                bad.append(tag + f": relative residual {res}")
            if not same(ds.b_after, b):
                bad.append(tag + ": db changed")
            if not (rs["kry_mdot"] > 0 and rs["kry_odot"] == 0 and rs["kry_it"] == info["its"]):
                bad.append(tag + f": routes {rs}")
            if size > 1 and not rs["kry_p_comb"] > 0:
                bad.append(tag + ": no rank-order combine ran")
            if rs["kry_p_xch"] != px * (info["its"] + info["restarts"] + 1):
                bad.append(tag + f": product exchanges {rs['kry_p_xch']}, px {px}")
            x2, info2, hist2 = ds.krylov(b, rtol=RTOL, restart=restart, maxit=MAXIT, partitioned=True, complete=True, check=False)
            if not (same(x2, x) and same(hist2, hist) and info2 == info):
                bad.append(tag + ": the second run differs")
            if not all_same((info, bits(hist).tolist(), bits(x).tolist())):
                bad.append(tag + ": info, hist or the completed x differ between the ranks")
            want = 0 if size == 1 else count_formula(info["its"], info["restarts"], cyc, px, 0, True)
            if st["collectives"] != want:
                bad.append(tag + f": {st['collectives']} collectives, the formula gives {want} (cyc {cyc}, px {px}, {info})")
            if not all_same(st):
                bad.append(tag + ": krylov_comm_stats differs between the ranks")
            stats[tag] = [st["collectives"], st["bytes"], info["its"], info["restarts"], cyc, px]
    oa.vc_halo(-1)
    # fused with a guess and without bit 3: the formula's other terms
    ds.solve(b, remove_mean=null, partitioned=True)
    cyc = oa.solve_comm_stats()["collectives"]
    px = 0 if size == 1 else (1 if foreign else 0)
    x, info, hist = ds.krylov(b, rtol=RTOL, restart=30, maxit=MAXIT, partitioned=True, x0=x0, check=False)
    st = oa.krylov_comm_stats()
    if info["rc"] != 0 or (size > 1 and info["its"] > 0 and
                           st["collectives"] != count_formula(info["its"], info["restarts"], cyc, px, 1, False)):
        bad.append(f"fused guess: {st}, {info}, cyc {cyc}, px {px}")
    if first[1]["rc"] != 0:
        bad.append(f"the first fused call: {first[1]}")
    ds.close()
    out.update(levels=h.nlevels, n0=n0, rows=[r0, r1], stats=stats)
    return bad


def exact_dots(V, w):
    """per column: (the correctly rounded sum of the exact products, sum |v_i w_i|), as
    tests/test_gpu_krylov.py takes them (Veltkamp / Dekker split of every product)"""
    def split(a):
        t = 134217729.0 * a
        hi = t - (t - a)
        return hi, a - hi
    p = V * w[:, None]
    vh, vl = split(V)
    wh, wl = split(w[:, None])
    e = ((vh * wh - p) + vh * wl + vl * wh) + vl * wl
    sums = np.array([math.fsum(np.concatenate([p[:, t], e[:, t]])) for t in range(V.shape[1])])
    return sums, np.abs(p).sum(axis=0)


def rank_order_sum(parts):
    """s = p_0; s = s + p_1; ... elementwise"""
    s = np.array(parts[0], dtype=np.float64)
    for p in parts[1:]:
        s = s + p
    return s


def run_combine(rank, size, out):
    """every rank runs the hook on its slice and the one-GPU hooks on the same slice (even ld,
    aligned base); the one-GPU values of all ranks, added in rank order in numpy, are the hook's
    bits.  A 1-row vector has no ragged cut and no cut with empty ranks between owners: n = 1
    takes the kinds that exist there"""
    bad = []
    u = 2.0 ** -53
    for n in (1, 257, 4097):
        rng = np.random.default_rng(n)
        V, w = rng.standard_normal((n, 17)), rng.standard_normal(n)
        sums, mags = exact_dots(V, w)
        bound = n * u / (1 - n * u) * mags
        for kind in pc.KINDS:
            try:
                s = pc.split(kind, n, size, seed=n)
            except (ValueError, AssertionError):
                if n == 1:
                    continue
                raise
            lo, hi = int(s[rank]), int(s[rank + 1])
            for nb in (1, 16, 17):
                tag = f"n={n} {kind} nb={nb}"
                Vo, wo = V[lo:hi, :nb], w[lo:hi]
                ld = (hi - lo + 1) & ~1
                got = oa.test_kry_mdot_ranks(Vo, wo)
                mine = oa.test_kry_mdot(Vo, wo, ld) if hi > lo else np.zeros(nb)     # no rows: +0
                parts = [None] * size
                dist.all_gather_object(parts, mine.tolist())
                want = rank_order_sum([np.array(p) for p in parts])
                if not same(got, want):
                    bad.append(tag + f": multi-dot {got} against {want}")
                if not np.all(np.abs(got - sums[:nb]) <= bound[:nb]):
                    bad.append(tag + ": multi-dot outside the bound of the exact sum")
                # the update's norm: w - V d on the slice, the partial sums of squares combined
                d = np.random.default_rng(nb).standard_normal(nb)
                wn, nrm = oa.test_kry_norm_ranks(Vo, wo, d)
                if hi > lo:
                    w1, n1 = oa.test_kry_update(Vo, wo, d, ld, norm=True)
                else:
                    w1, n1 = np.zeros(0), np.zeros(2)
                if not same(wn, w1):
                    bad.append(tag + ": the updated slice differs")
                dist.all_gather_object(parts, [float(n1[0])])
                wsum = rank_order_sum([np.array(p) for p in parts])[0]
                if not (same(nrm[0], wsum) and same(nrm[1], np.sqrt(wsum))):
                    bad.append(tag + f": norm {nrm} against {wsum}")
                wall = [None] * size
                dist.all_gather_object(wall, wn.tolist())
                wfull = np.concatenate([np.array(q, dtype=np.float64) for q in wall])
                es, em = exact_dots(wfull[:, None], wfull)
                if not abs(nrm[0] - es[0]) <= n * u / (1 - n * u) * em[0]:
                    bad.append(tag + ": norm outside the bound of the exact sum")
    return bad


def run_product(rank, size, out):
    bad = []
    for kind, seed in [(k, s) for k in pc.KINDS for s in range(3)]:
        rng = np.random.default_rng(200 + seed)
        rn, cn = 301, 257
        M = pc.with_row_lengths(rng, rn, cn, rng.integers(0, 9, rn))
        rs, vs = pc.split(kind, rn, size, seed), pc.split(kind, cn, size, seed + 7)
        truth = rng.standard_normal(cn)
        cols = M.col[M.row_off[rs[rank]]:M.row_off[rs[rank + 1]]]
        z = np.full(cn, POISON)                  # the truth on the own and the referenced entries
        z[vs[rank]:vs[rank + 1]] = truth[vs[rank]:vs[rank + 1]]
        want_z = z.copy()
        for idx in refsolve_part.halo_lists(cols, vs, rank).values():
            want_z[idx] = truth[idx]
        got, z_after = oa.test_kry_spmv_part(M, rs, vs, z)
        want = refsolve.apply_M(abi.Csr(M.rn, M.cn, M.row_off, M.col, M.a), truth)[rs[rank]:rs[rank + 1]]
        d = pc.diff_vec(got, want)
        if d:
            bad.append(f"{kind} seed {seed}: own rows {d}")
        d = pc.diff_vec(z_after, want_z)
        if d:
            bad.append(f"{kind} seed {seed}: the operand {d}")
    return bad


def crs_krylov_ranks(h, ids, b, x0, guess, **kw):
    """amgd_crs_krylov on several ranks: b assembled as refsolve_part.crs_solve_ranks assembles
    it (+0 + g_0 + g_1 + ... in rank order), the guess of an id x0 at the first local dof of the
    lowest rank that carries it, refkrylov.fgmres, x to every local dof of every rank"""
    n0 = int(h.levels[0].n)
    g = np.zeros(n0)
    for r in range(len(ids)):
        g = g + refsolve_part.partial_sums(n0, ids[r], b[r])
    xg = None
    if guess:
        xg = np.zeros(n0)
        seen = np.zeros(n0, dtype=bool)
        for r in range(len(ids)):
            for k, i in enumerate(np.asarray(ids[r], dtype=np.int64)):
                if i and not seen[i - 1]:
                    seen[i - 1] = True
                    xg[i - 1] = x0[r][k]
    res = refkrylov.fgmres(h, g, x0=xg, **kw)
    xs = []
    for r in range(len(ids)):
        idr = np.asarray(ids[r], dtype=np.int64)
        x = np.array(x0[r], dtype=np.float64)
        x[idr != 0] = res["x"][idr[idr != 0] - 1]
        xs.append(x)
    return res, xs


def run_crs(rank, size, out):
    L = oa.lib()
    ranks, n0, null = psw.crs_case(os.environ["PK_CASE"], size)
    n, ids, Ai, Aj, Av, b, _ = ranks[rank]
    x0s = [np.random.default_rng(50 + r).standard_normal(q[0]) for r, q in enumerate(ranks)]   # differ between ranks
    bad = []
    kw = dict(rtol=RTOL, restart=30, maxit=MAXIT)
    for mode in ("partitioned", "replicated"):
        L.amgd_comm_set_partitioned(1 if mode == "partitioned" else 0)
        hd = abi.crs_setup(L, n, ids, Ai, Aj, Av, null_space=null, rank=rank, np_=size)
        if hd is None:
            return [mode + ": crs_setup returned NULL"]
        h = abi.crs_export(L, hd)
        for guess in (False, True):
            tag = f"{mode} guess={int(guess)}"
            x, info = abi.crs_krylov(L, hd, b, x0=x0s[rank], ordered=True, guess=guess, **kw)
            if not same(abi.crs_krylov.b_after, b):
                bad.append(tag + ": b modified")
            want, xs = crs_krylov_ranks(h, [q[1] for q in ranks], [q[5] for q in ranks], x0s, guess, **kw)
            if info_diff(info, want):
                bad.append(tag + f": info differs in {info_diff(info, want)}: {info}")
                continue
            d = pc.diff_vec(x, xs[rank])
            if d:
                bad.append(f"{tag}: x {d}")
            if not (same(x[n - 3:n - 1], x0s[rank][n - 3:n - 1]) and same(x[n - 1:], x[:1])):
                bad.append(tag + ": id-0 dofs or the repeated dof")
        L.crs_free(hd)
    return bad


def main():
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    oa.init(0)
    L = oa.lib()
    L.amgd_test_pool_inuse.restype = C.c_uint64
    before = L.amgd_test_pool_inuse()
    shard.init_host(rank, size)
    what = os.environ["PK_WHAT"]
    out = {"rank": rank, "size": size, "what": what}
    if what != "crs":
        L.amgd_comm_set_partitioned(1)
    bad = {"solve": run_solve, "combine": run_combine, "product": run_product, "crs": run_crs}[what](rank, size, out)
    # after close() / crs_free nothing of the solve stays on the device
    out["leak_bytes"] = int(L.amgd_test_pool_inuse()) - int(before)
    out["bad"] = bad[:12]
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not bad and out["leak_bytes"] == 0 else 1)


if __name__ == "__main__":
    main()
