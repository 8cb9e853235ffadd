"""V-cycle benchmark: builds the 7-point Poisson hierarchy of an n^3 grid on the GPU and times
amgd_solve_device on it -- the default routing of the fused kernels, the same with the
cooperative long-row kernels, with the one-workgroup tail by rows alone, without the tail,
and the composed path (only kernels the setup already had: the baseline).

Method: every configuration is warmed up, then timed in windows of at least --seconds of
cycles with device events (amgd_solve_stats) around them; the configurations alternate
inside each of --repeats rounds in one process, and the spread over the rounds is reported
next to the median.  All configurations must return the same bits.  Prints one JSON line:
ms per cycle (median, min, max) per configuration, algorithmic bytes per cycle (12 B per
matrix entry per pass + 8 B per vector element read or written), the share of 8 TB/s those
bytes over the median time amount to (a bandwidth bound), and launches per cycle -- nominal:
the library tallies them per product from the form it took, not at the launch sites.

--mode part: the partitioned cycle on one rank (a one-rank RCCL communicator in partitioned
mode, as bench.py --mode part) against the one-GPU cycle of the same tree: both hierarchies
are set up in this process and their cycles alternate inside each round, default routing;
part_n1_repl0 distributes every level but the bottom one.  The same bits are required.

--nrhs 2,4,8: the multi-RHS cycle.  For every listed K one amgd_solve_device_n call of K columns
(groups of K only) is timed against K single default-routed cycles, in the same process and
the same alternating rounds: with the kernel family by row shape, with the long-row kernels
on every shape and with the short-row kernels on every shape.  Reported per configuration:
ms per call and per column (median, min, max over the rounds), the ratio of the per-column
time to the single cycle of this run, the algorithmic bytes (matrices once per group -- those
of a level that falls back column by column once per column --, vectors per column) and
their share of 8 TB/s, launches per call, and `wins`: the per-column median beats the single
cycle's median by more than the larger of the two min-max spreads.  Every configuration must
return the single cycle's bits column by column: asserted.

--krylov: flexible GMRES around the cycle (amgd_krylov_device) on b = A x*, rtol 1e-8, restart 30.
Whole solves with the fused dots and with the ordered dots, and the floor of an inner iteration
-- one cycle plus one level-0 product, nothing else -- alternate inside each round in the same
process; device events around every call (amgd_krylov_stats).  Reported: ms per inner iteration
(median, min, max over the rounds) per path, iterations, the relative residual recomputed on
the host, the floor, the share of an iteration spent outside the cycle and the product, and
`fused_wins`: the fused median beats the ordered one by more than the larger min-max spread.

--krylov --mode part: the fused solve on a one-rank RCCL communicator in partitioned mode against
the one-GPU fused solve of the same matrix, alternating inside each round; ms per inner iteration,
median [min, max], and whether the two gave the same bits.

--krylov --nrhs 2,4,8: the multi-RHS solver.  For every listed K one amgd_krylov_device_n call of
K columns (K slots; fused dots; the product's kernel family by row shape and, `_long`, the
long-row kernel forced) against the same columns solved one by one with amgd_krylov_device on
the same device blocks, alternating inside each round in one process, device events around every
call.  Reported per configuration: ms per column per inner iteration (median, min, max over the
rounds), its ratio to the single solver of this run, the floor (K cycles and K products in a
step's groups, per column), the share of a column iteration spent outside the cycle and the
product, the route counters of one call, the bytes the product's operand copies move per
iteration, and `wins`: the median beats the single solver's by more than the larger min-max
spread.  Every column must come out with the single solver's bits: asserted.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omp_amg_amd as oa  # noqa: E402
from omp_amg_amd import problems  # noqa: E402

HBM_BYTES_PER_S = 8e12

CONFIGS = {                      # fused, coop, tail (-1: the library's defaults)
    "fused": (1, -1, -1),        # the default routing
    "fused_coop": (1, 1, -1),    # long-row shapes through the cooperative kernels
    "fused_tail1024": (1, -1, 1024),   # the tail by rows alone, whatever its levels' work
    "fused_notail": (1, -1, 0),
    "composed": (0, 0, 0),       # the baseline: only kernels the setup already had
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=("one", "part"), default="one")
    ap.add_argument("--nrhs", default="", help="group sizes out of 2,4,8: time the multi-RHS cycle")
    ap.add_argument("--krylov", action="store_true", help="time flexible GMRES around the cycle")
    a = ap.parse_args()
    if a.krylov and a.nrhs:
        return main_krylov_nrhs(a)
    if a.krylov and a.mode == "part":
        return main_krylov_part(a)
    if a.krylov:
        return main_krylov(a)
    if a.nrhs:
        return main_nrhs(a)
    if a.mode == "part":
        return main_part(a)

    oa.init()
    L = oa.lib()
    L.amgd_test_vc_launches.restype = C.c_uint64
    ds = oa.DeviceSetup(*problems.poisson3d(a.n))
    st = ds.run()
    n0 = a.n ** 3
    b = np.random.default_rng(1).standard_normal(n0)
    ds.vectors(n0)
    L.amgd_dev_upload(ds.db, b.ctypes.data, b.nbytes)

    def select(cfg):
        fused, coop, tail = CONFIGS[cfg]
        oa.vc_fused(fused)
        oa.vc_coop(coop)
        oa.vc_tail(tail)

    def cycles(k):
        """k cycles; device-event ms per cycle, launches per cycle"""
        s0, l0 = oa.solve_stats(), L.amgd_test_vc_launches()
        for _ in range(k):
            rc = L.amgd_solve_device(ds.h, ds.dx, ds.db, 0)
            if rc != 0:
                raise RuntimeError(f"amgd_solve_device rc={rc}")
        L.amgd_dev_sync()
        s1 = oa.solve_stats()
        return (s1["ms"] - s0["ms"]) / k, (L.amgd_test_vc_launches() - l0) / k

    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "setup_ms": st["t_total_ms"]}
    xs, count, launches, routes = {}, {}, {}, {}
    for cfg in CONFIGS:
        select(cfg)
        cycles(a.warmup)
        x = np.empty(n0)
        L.amgd_dev_download(x.ctypes.data, ds.dx, x.nbytes)
        xs[cfg] = x
        ms, _ = cycles(10)
        count[cfg] = max(10, int(a.seconds * 1e3 / max(ms, 1e-3)) + 1)
        oa.route_stats()
        _, launches[cfg] = cycles(1)
        r = oa.route_stats()
        routes[cfg] = {k: r[k] for k in ("vc_thr", "vc_wave", "vc_comp", "vc_tail")}
    same = all(np.array_equal(xs["composed"].view(np.uint64), x.view(np.uint64)) for x in xs.values())
    times = {cfg: [] for cfg in CONFIGS}
    for _ in range(a.repeats):
        for cfg in CONFIGS:
            select(cfg)
            times[cfg].append(cycles(count[cfg])[0])
    by = oa.solve_stats()["bytes"]
    out["bytes_per_cycle"] = by
    out["same_bits"] = bool(same)
    for cfg in CONFIGS:
        t = sorted(times[cfg])
        med = t[len(t) // 2]
        out[cfg] = {"ms": med, "ms_min": t[0], "ms_max": t[-1], "cycles_per_window": count[cfg],
                    "launches": launches[cfg], "routes": routes[cfg],
                    "share_of_8TBs_bandwidth_bound": by / (med * 1e-3) / HBM_BYTES_PER_S}
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)
    ds.close()
    print(json.dumps(out))
    return 0 if same else 1


def main_part(a):
    from omp_amg_amd import shard
    oa.init()
    L = oa.lib()
    L.amgd_test_vc_launches.restype = C.c_uint64
    n0 = a.n ** 3
    coo = problems.poisson3d(a.n)
    b = np.random.default_rng(1).standard_normal(n0)
    one = oa.DeviceSetup(*coo)
    st = one.run()
    shard.init_rccl(0, 1)
    L.amgd_comm_set_partitioned(1)
    part = oa.DeviceSetup(*coo)
    part.run()
    for ds in (one, part):
        ds.vectors(n0)
        L.amgd_dev_upload(ds.db, b.ctypes.data, b.nbytes)
    configs = {"one_gpu": (one, -1), "part_n1": (part, -1), "part_n1_repl0": (part, 0)}

    def cycles(cfg, k):
        ds, repl = configs[cfg]
        oa.vc_repl(repl)
        s0, l0 = oa.solve_stats(), L.amgd_test_vc_launches()
        for _ in range(k):
            rc = L.amgd_solve_device(ds.h, ds.dx, ds.db, 4 if ds is part else 0)
            if rc != 0:
                raise RuntimeError(f"amgd_solve_device rc={rc}")
        L.amgd_dev_sync()
        s1 = oa.solve_stats()
        return (s1["ms"] - s0["ms"]) / k, (L.amgd_test_vc_launches() - l0) / k

    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "mode": "part"}
    xs, count, launches, routes, by = {}, {}, {}, {}, {}
    for cfg, (ds, _) in configs.items():
        cycles(cfg, a.warmup)
        x = np.empty(n0)
        L.amgd_dev_download(x.ctypes.data, ds.dx, x.nbytes)
        xs[cfg] = x
        ms, _ = cycles(cfg, 10)
        count[cfg] = max(10, int(a.seconds * 1e3 / max(ms, 1e-3)) + 1)
        oa.route_stats()
        _, launches[cfg] = cycles(cfg, 1)
        r = oa.route_stats()
        routes[cfg] = {k: r[k] for k in ("vc_thr", "vc_wave", "vc_comp", "vc_tail", "vc_halo", "vc_allg", "vc_repl")}
        by[cfg] = oa.solve_stats()["bytes"]
    same = all(np.array_equal(xs["one_gpu"].view(np.uint64), x.view(np.uint64)) for x in xs.values())
    times = {cfg: [] for cfg in configs}
    for _ in range(a.repeats):
        for cfg in configs:
            times[cfg].append(cycles(cfg, count[cfg])[0])
    out["same_bits"] = bool(same)
    for cfg in configs:
        t = sorted(times[cfg])
        med = t[len(t) // 2]
        out[cfg] = {"ms": med, "ms_min": t[0], "ms_max": t[-1], "cycles_per_window": count[cfg],
                    "launches": launches[cfg], "routes": routes[cfg], "bytes_per_cycle": by[cfg],
                    "share_of_8TBs_bandwidth_bound": by[cfg] / (med * 1e-3) / HBM_BYTES_PER_S}
    oa.vc_repl(-1)
    one.close()
    part.close()
    shard.free()
    print(json.dumps(out))
    return 0 if same else 1


def main_nrhs(a):
    ks = [int(k) for k in a.nrhs.split(",")]
    if not ks or any(k not in (2, 4, 8) for k in ks):
        raise SystemExit("--nrhs takes group sizes out of 2,4,8")
    oa.init()
    L = oa.lib()
    L.amgd_test_vc_launches.restype = C.c_uint64
    ds = oa.DeviceSetup(*problems.poisson3d(a.n))
    st = ds.run()
    n0 = a.n ** 3
    kmax = max(ks)
    B = np.random.default_rng(1).standard_normal((n0, kmax))
    for f in (oa.vc_fused, oa.vc_coop, oa.vc_tail):
        f(-1)
    ref = np.stack([ds.solve(B[:, j]) for j in range(kmax)], axis=1)     # the single cycle's bits
    oa.vc_mrhs_k(ks)
    ds.solve_n(B)                           # the device blocks ds.dbn / ds.dxn (ld = n0), B uploaded
    configs = ["single"] + [f"k{k}_{fam}" for k in ks for fam in ("auto", "long", "short")]

    def select(cfg):
        if cfg != "single":
            k, fam = cfg[1:].split("_")
            oa.vc_mrhs_k((int(k),))
            oa.vc_mrhs_family(fam)

    def calls(cfg, reps):
        """reps calls; device-event ms per call, launches per call"""
        l0 = L.amgd_test_vc_launches()
        if cfg == "single":
            s0 = oa.solve_stats()["ms"]
            for _ in range(reps):
                rc = L.amgd_solve_device(ds.h, ds.dx, ds.db, 0)
                assert rc == 0, rc
            L.amgd_dev_sync()
            ms = oa.solve_stats()["ms"] - s0
        else:
            k = int(cfg[1:].split("_")[0])
            s0 = oa.solve_n_stats()["ms"]
            for _ in range(reps):
                rc = L.amgd_solve_device_n(ds.h, ds.dxn, ds.dbn, k, n0, 0)
                assert rc == 0, rc
            L.amgd_dev_sync()
            ms = oa.solve_n_stats()["ms"] - s0
        return ms / reps, (L.amgd_test_vc_launches() - l0) / reps

    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "mode": "nrhs"}
    count, launches, routes, by = {}, {}, {}, {}
    for cfg in configs:
        select(cfg)
        calls(cfg, a.warmup)
        if cfg != "single":
            k = int(cfg[1:].split("_")[0])
            X = np.empty((kmax, n0))
            L.amgd_dev_download(X.ctypes.data, ds.dxn, k * n0 * 8)
            for j in range(k):
                assert np.array_equal(X[j].view(np.uint64), ref[:, j].view(np.uint64)), (cfg, j)
        ms, _ = calls(cfg, 5)
        count[cfg] = max(5, int(a.seconds * 1e3 / max(ms, 1e-3)) + 1)
        oa.route_stats()
        _, launches[cfg] = calls(cfg, 1)
        r = oa.route_stats()
        routes[cfg] = {q: r[q] for q in ("vc_thr", "vc_comp", "vc_tail", "vc_mr_thr", "vc_mr_wave", "vc_mr_single", "vc_mr_comp")}
        by[cfg] = oa.solve_stats()["bytes"] if cfg == "single" else oa.solve_n_stats()["bytes"]
    times = {cfg: [] for cfg in configs}
    for _ in range(a.repeats):
        for cfg in configs:
            select(cfg)
            times[cfg].append(calls(cfg, count[cfg])[0])
    out["same_bits"] = True
    ts = sorted(times["single"])
    smed, sspread = ts[len(ts) // 2], ts[-1] - ts[0]
    for cfg in configs:
        t = sorted(times[cfg])
        med = t[len(t) // 2]
        k = 1 if cfg == "single" else int(cfg[1:].split("_")[0])
        out[cfg] = {"ms": med, "ms_min": t[0], "ms_max": t[-1], "ms_per_column": med / k,
                    "ratio_to_single": med / k / smed, "calls_per_window": count[cfg],
                    "launches": launches[cfg], "routes": routes[cfg], "bytes": by[cfg],
                    "share_of_8TBs_bandwidth_bound": by[cfg] / (med * 1e-3) / HBM_BYTES_PER_S,
                    "wins": bool(smed - med / k > max(sspread, (t[-1] - t[0]) / k))}
    oa.vc_mrhs_k(-1)
    oa.vc_mrhs_family(-1)
    ds.close()
    print(json.dumps(out))
    return 0


def main_krylov(a):
    oa.init()
    L = oa.lib()
    L.amgd_test_kry_floor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.amgd_test_kry_floor.restype = C.c_int
    Ai, Aj, Av = problems.poisson3d(a.n)
    ds = oa.DeviceSetup(Ai, Aj, Av)
    st = ds.run()
    n0 = a.n ** 3
    xs = np.random.default_rng(5).standard_normal(n0)
    b = np.bincount(Ai.astype(np.int64), weights=Av * xs[Aj.astype(np.int64)], minlength=n0)
    rtol, restart = 1e-8, 30
    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "mode": "krylov", "rtol": rtol, "restart": restart}
    configs = ("fused", "ordered", "floor")
    info = {}
    for cfg in configs[:2]:                  # warm-up: the plan, the workspace, the residual on the host
        x, info[cfg], _ = ds.krylov(b, rtol=rtol, restart=restart, ordered=cfg == "ordered")
        r = b - np.bincount(Ai.astype(np.int64), weights=Av * x[Aj.astype(np.int64)], minlength=n0)
        info[cfg]["relres_host"] = float(np.linalg.norm(r) / np.linalg.norm(b))
    o = {cfg: abi_opts(rtol, restart, cfg == "ordered") for cfg in configs[:2]}

    def window(cfg, reps):
        """reps calls; device-event ms per inner iteration (floor: per call)"""
        s0 = oa.krylov_stats()
        for _ in range(reps):
            if cfg == "floor":
                rc = L.amgd_test_kry_floor(ds.h, ds.dx, ds.db)
            else:
                ki = oa.abi.KrylovInfo()
                rc = L.amgd_krylov_device(ds.h, ds.dx, ds.db, C.byref(o[cfg]), C.byref(ki), None, 0)
            assert rc == 0, (cfg, rc)
        L.amgd_dev_sync()
        s1 = oa.krylov_stats()
        return (s1["ms"] - s0["ms"]) / (reps if cfg == "floor" else s1["its"] - s0["its"])

    count = {}
    for cfg in configs:
        window(cfg, a.warmup if cfg == "floor" else 1)
        reps0 = 10 if cfg == "floor" else 1
        ms = window(cfg, reps0) * (1 if cfg == "floor" else info[cfg]["its"])
        count[cfg] = max(reps0, int(a.seconds * 1e3 / max(ms, 1e-3)) + 1)
    times = {cfg: [] for cfg in configs}
    for _ in range(a.repeats):
        for cfg in configs:
            times[cfg].append(window(cfg, count[cfg]))
    med, spread = {}, {}
    for cfg in configs:
        t = sorted(times[cfg])
        med[cfg], spread[cfg] = t[len(t) // 2], t[-1] - t[0]
        out[cfg] = {"ms_per_iteration": med[cfg], "ms_min": t[0], "ms_max": t[-1], "calls_per_window": count[cfg]}
    for cfg in info:
        out[cfg].update({k: info[cfg][k] for k in ("rc", "its", "restarts", "cycles", "relres_host")})
        out[cfg]["share_outside_cycle_and_product"] = 1 - med["floor"] / med[cfg]
    out["fused_wins"] = bool(med["ordered"] - med["fused"] > max(spread["ordered"], spread["fused"]))
    ds.close()
    print(json.dumps(out))
    return 0


def main_krylov_part(a):
    """--krylov --mode part: the fused solve on a one-rank RCCL communicator in partitioned mode
    (amgd_krylov_device with flag bit 2) against the one-GPU fused solve of the same matrix, the
    two alternating inside each round as main_part does for the cycle; ms per inner iteration"""
    from omp_amg_amd import shard
    oa.init()
    L = oa.lib()
    Ai, Aj, Av = problems.poisson3d(a.n)
    n0 = a.n ** 3
    xs = np.random.default_rng(5).standard_normal(n0)
    b = np.bincount(Ai.astype(np.int64), weights=Av * xs[Aj.astype(np.int64)], minlength=n0)
    rtol, restart = 1e-8, 30
    one = oa.DeviceSetup(Ai, Aj, Av)
    st = one.run()
    shard.init_rccl(0, 1)
    L.amgd_comm_set_partitioned(1)
    part = oa.DeviceSetup(Ai, Aj, Av)
    part.run()
    configs = {"one_gpu": one, "part_n1": part}
    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "mode": "krylov_part", "rtol": rtol, "restart": restart}
    xsol, info = {}, {}
    for cfg, ds in configs.items():          # warm-up: the plan, the workspace
        xsol[cfg], info[cfg], _ = ds.krylov(b, rtol=rtol, restart=restart, partitioned=ds is part)
    same = bool(np.array_equal(xsol["one_gpu"].view(np.uint64), xsol["part_n1"].view(np.uint64))
                and info["one_gpu"] == info["part_n1"])
    o = {cfg: oa.abi.KrylovOpts(rtol, 0.0, restart, 0, 4 if ds is part else 0) for cfg, ds in configs.items()}

    def window(cfg, reps):
        ds = configs[cfg]
        s0 = oa.krylov_stats()
        for _ in range(reps):
            ki = oa.abi.KrylovInfo()
            rc = L.amgd_krylov_device(ds.h, ds.dx, ds.db, C.byref(o[cfg]), C.byref(ki), None, 0)
            assert rc == 0, (cfg, rc)
        L.amgd_dev_sync()
        s1 = oa.krylov_stats()
        return (s1["ms"] - s0["ms"]) / (s1["its"] - s0["its"])

    count = {}
    for cfg in configs:
        window(cfg, 1)
        ms = window(cfg, 1) * info[cfg]["its"]
        count[cfg] = max(1, int(a.seconds * 1e3 / max(ms, 1e-3)) + 1)
    times = {cfg: [] for cfg in configs}
    for _ in range(a.repeats):
        for cfg in configs:
            times[cfg].append(window(cfg, count[cfg]))
    out["same_bits"] = same
    for cfg in configs:
        t = sorted(times[cfg])
        out[cfg] = {"ms_per_iteration": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1], "calls_per_window": count[cfg],
                    "its": info[cfg]["its"], "rc": info[cfg]["rc"]}
    out["gap"] = out["part_n1"]["ms_per_iteration"] / out["one_gpu"]["ms_per_iteration"] - 1
    one.close()
    part.close()
    shard.free()
    print(json.dumps(out))
    return 0 if same else 1


def main_krylov_nrhs(a):
    ks = [int(k) for k in a.nrhs.split(",")]
    if not ks or any(k not in (2, 4, 8) for k in ks):
        raise SystemExit("--nrhs takes column counts out of 2,4,8")
    oa.init()
    L = oa.lib()
    L.amgd_test_kry_floor_n.argtypes = [C.c_void_p, C.c_int]
    L.amgd_test_kry_floor_n.restype = C.c_int
    Ai, Aj, Av = problems.poisson3d(a.n)
    ds = oa.DeviceSetup(Ai, Aj, Av)
    st = ds.run()
    n0, kmax = a.n ** 3, max(ks)
    rng = np.random.default_rng(5)
    ii, jj = Ai.astype(np.int64), Aj.astype(np.int64)
    B = np.stack([np.bincount(ii, weights=Av * rng.standard_normal(n0)[jj], minlength=n0) for _ in range(kmax)], axis=1)
    rtol, restart = 1e-8, 30
    o = abi_opts(rtol, restart, False)
    out = {"n": a.n, "rows": n0, "levels": st["nlevels"], "mode": "krylov_nrhs", "rtol": rtol, "restart": restart}
    oa.vc_mrhs_k((2, 4, 8))
    oa.kry_slots(kmax)
    X, infos, _ = ds.krylov_n(B, rtol=rtol, restart=restart)        # the device blocks (ld = n0), the slots
    assert ds.rc_n == 0, ds.rc_n
    its = [i["its"] for i in infos]
    ref = np.empty((kmax, n0))
    for j in range(kmax):                                            # the single solver's bits, same pointers
        ki = oa.abi.KrylovInfo()
        rc = L.amgd_krylov_device(ds.h, ds.dxn + j * n0 * 8, ds.dbn + j * n0 * 8, C.byref(o), C.byref(ki), None, 0)
        assert rc == 0 and ki.its == its[j], (j, rc, ki.its, its[j])
    L.amgd_dev_sync()
    L.amgd_dev_download(ref.ctypes.data, ds.dxn, ref.nbytes)
    assert np.array_equal(ref.view(np.uint64), np.ascontiguousarray(X.T).view(np.uint64))
    configs = ["single"] + [f"k{k}{fam}" for k in ks for fam in ("", "_long")] + [f"floor{k}" for k in ks]

    def kof(cfg):
        return int(cfg.replace("floor", "").replace("k", "").split("_")[0])

    def select(cfg):
        oa.kry_family("long" if cfg.endswith("_long") else "auto")
        if cfg != "single":
            oa.kry_slots(kof(cfg))

    def window(cfg, reps):
        """reps rounds over the configuration's columns; device-event ms per column iteration
        (floor: per column)"""
        if cfg == "single":
            s0 = oa.krylov_stats()
            for _ in range(reps):
                for j in range(kmax):
                    ki = oa.abi.KrylovInfo()
                    rc = L.amgd_krylov_device(ds.h, ds.dxn + j * n0 * 8, ds.dbn + j * n0 * 8, C.byref(o), C.byref(ki),
                                              None, 0)
                    assert rc == 0, (cfg, j, rc)
            L.amgd_dev_sync()
            s1 = oa.krylov_stats()
            return (s1["ms"] - s0["ms"]) / (s1["its"] - s0["its"])
        k = kof(cfg)
        s0 = oa.krylov_n_stats()["ms"]
        kis = (oa.abi.KrylovInfo * k)()
        for _ in range(reps):
            if cfg.startswith("floor"):
                rc = L.amgd_test_kry_floor_n(ds.h, k)
            else:
                rc = L.amgd_krylov_device_n(ds.h, ds.dxn, ds.dbn, k, n0, C.byref(o), kis, None, None, 0)
            assert rc == 0, (cfg, rc)
        L.amgd_dev_sync()
        ms = oa.krylov_n_stats()["ms"] - s0
        return ms / (reps * (k if cfg.startswith("floor") else sum(its[:k])))

    count, routes = {}, {}
    for cfg in configs:
        select(cfg)
        window(cfg, a.warmup if cfg.startswith("floor") else 1)
        if cfg[0] == "k":                       # the bits of this configuration
            k = kof(cfg)
            got = np.empty((k, n0))
            L.amgd_dev_download(got.ctypes.data, ds.dxn, got.nbytes)
            assert np.array_equal(got.view(np.uint64), ref[:k].view(np.uint64)), cfg
        oa.route_stats()
        per = window(cfg, 1)
        r = oa.route_stats()
        routes[cfg] = {q: r[q] for q in ("kry_it", "kry_n_step", "kry_n_mixed", "kry_n_prod", "kry_n_single",
                                         "vc_mr_thr", "vc_mr_wave", "vc_mr_single")}
        units = kof(cfg) if cfg.startswith("floor") else sum(its[:kof(cfg)]) if cfg != "single" else sum(its)
        count[cfg] = max(1, int(a.seconds * 1e3 / max(per * units, 1e-3)) + 1)
    times = {cfg: [] for cfg in configs}
    for _ in range(a.repeats):
        for cfg in configs:
            select(cfg)
            times[cfg].append(window(cfg, count[cfg]))
    out["same_bits"] = True
    out["its"] = its
    ts = sorted(times["single"])
    smed, sspread = ts[len(ts) // 2], ts[-1] - ts[0]
    for cfg in configs:
        t = sorted(times[cfg])
        med = t[len(t) // 2]
        out[cfg] = {"ms_per_column_iteration": med, "ms_min": t[0], "ms_max": t[-1], "calls_per_window": count[cfg],
                    "routes": routes[cfg]}
        if cfg[0] == "k":
            k = kof(cfg)
            fl = sorted(times[f"floor{k}"])
            out[cfg].update({"ratio_to_single": med / smed,
                             "share_outside_cycle_and_product": 1 - fl[len(fl) // 2] / med,
                             "operand_copy_bytes_per_product": 16 * n0 * k,
                             "wins": bool(smed - med > max(sspread, t[-1] - t[0]))})
    for f in (oa.vc_mrhs_k, oa.kry_slots, oa.kry_family):
        f(-1)
    ds.close()
    print(json.dumps(out))
    return 0


def abi_opts(rtol, restart, ordered):
    return oa.abi.KrylovOpts(rtol, 0.0, restart, 0, 1 if ordered else 0)


if __name__ == "__main__":
    sys.exit(main())
