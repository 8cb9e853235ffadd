#!/usr/bin/env python3
"""Collectives and bytes per cycle of the partitioned V-cycle (DESIGN.md "Solve", the
partitioned part): N processes on one GPU over the host transport set up the 7-point m^3
hierarchy row-partitioned, then run one cycle per exchange mode (halo / allgather) with the
replication limit at its default and at 0, and report amgd_solve_comm_stats -- COUNTS from
the plan's lists, not times: host-transport times say nothing about xGMI.  Every mode's own
rows must equal the first mode's bit for bit.  Also prints the plan's levels (first position,
F points, matrix entries per cycle, summed over the ranks for distributed levels), the figures
the replication default is reasoned from.

--krylov: instead, one fused flexible GMRES solve (amgd_krylov_device with flag bit 2, b = A x*,
rtol 1e-8, restart 30) per exchange mode, and amgd_krylov_comm_stats: collectives and bytes of
the call and per inner iteration, one cycle's share, and the documented count formula.

usage: python tools/part_solve_counts.py <m> <N> [out.json] [--krylov]"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = [("default", -1, 1), ("default", -1, 0), ("0", 0, 1), ("0", 0, 0)]   # (name, limit, halo)


def levels(L, h):
    L.amgd_test_vc_plan_levels.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * (4 * 64))()
    n = L.amgd_test_vc_plan_levels(h, buf, 64)
    return [[int(buf[4 * l + k]) for k in range(4)] for l in range(n)]


def rank_main(m):
    import numpy as np
    import torch.distributed as dist
    import omp_amg_amd as oa
    from omp_amg_amd import problems, shard
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    oa.init(0)
    shard.init_host(rank, size)
    L = oa.lib()
    L.amgd_comm_set_partitioned(1)
    n = m ** 3
    ds = oa.DeviceSetup(*problems.poisson3d(m, 7, rows_range=(rank * n // size, (rank + 1) * n // size)))
    st = ds.run()
    r0, r1 = ds.rows()
    b = np.random.default_rng(1).standard_normal(n)
    out = {"rank": rank, "levels": int(st["nlevels"]), "rows": [r0, r1], "modes": []}
    first = None
    for name, limit, halo in MODES:
        oa.vc_repl(limit)
        oa.vc_halo(halo)
        x = ds.solve(b, partitioned=True)[r0:r1]
        cs = oa.solve_comm_stats()
        first = x if first is None else first
        out["modes"].append({"replication": name, "exchange": "halo" if halo else "allgather",
                             "collectives": cs["collectives"], "bytes_sent_all_ranks": cs["bytes"],
                             "same_bits": bool(np.array_equal(x.view(np.uint64), first.view(np.uint64))),
                             "plan_levels": levels(L, ds.h)})
    ds.close()
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


def rank_main_krylov(m):
    import numpy as np
    import torch.distributed as dist
    import omp_amg_amd as oa
    from omp_amg_amd import problems, shard
    rank, size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=size)
    oa.init(0)
    shard.init_host(rank, size)
    oa.lib().amgd_comm_set_partitioned(1)
    n = m ** 3
    ds = oa.DeviceSetup(*problems.poisson3d(m, 7, rows_range=(rank * n // size, (rank + 1) * n // size)))
    st = ds.run()
    r0, r1 = ds.rows()
    Ai, Aj, Av = problems.poisson3d(m)
    xs = np.random.default_rng(5).standard_normal(n)
    b = np.bincount(Ai.astype(np.int64), weights=Av * xs[Aj.astype(np.int64)], minlength=n)
    out = {"rank": rank, "levels": int(st["nlevels"]), "rows": [r0, r1], "modes": []}
    for halo in (1, 0):
        oa.vc_halo(halo)
        ds.solve(b, partitioned=True)
        cyc = oa.solve_comm_stats()
        oa.route_stats()
        x, info, _ = ds.krylov(b, rtol=1e-8, restart=30, partitioned=True, complete=True)
        cs, rs = oa.krylov_comm_stats(), oa.route_stats()
        res = float(np.linalg.norm(b - np.bincount(Ai.astype(np.int64), weights=Av * x[Aj.astype(np.int64)], minlength=n))
                    / np.linalg.norm(b))
        its = max(info["its"], 1)
        px = 1 if rs["kry_p_xch"] else 0
        out["modes"].append({"exchange": "halo" if halo else "allgather", "rc": info["rc"], "its": info["its"],
                             "restarts": info["restarts"], "relres_host": res,
                             "collectives": cs["collectives"], "bytes_sent_all_ranks": cs["bytes"],
                             "collectives_per_iteration": cs["collectives"] / its,
                             "bytes_per_iteration": cs["bytes"] / its,
                             "cycle_collectives": cyc["collectives"], "cycle_bytes": cyc["bytes"],
                             "product_exchanges": rs["kry_p_xch"], "combines": rs["kry_p_comb"],
                             "formula": 1 + info["its"] * (cyc["collectives"] + px + 3)
                             + (info["restarts"] + 1) * (px + 1) + 1})
    ds.close()
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


def main_krylov(a, ps):
    ranks = collect(a, ps)
    modes = []
    for k in range(2):
        ms = [r["modes"][k] for r in ranks]
        modes.append(dict(ms[0], agree_across_ranks=all(x == ms[0] for x in ms),
                          matches_formula=ms[0]["collectives"] == ms[0]["formula"]))
    res = {"workload": f"3D 7-point Poisson {a.m}^3, flexible GMRES (fused), rtol 1e-8, restart 30", "ranks": a.N,
           "levels": ranks[0]["levels"], "modes": modes,
           "transport": "host (gloo, N processes on one GPU): counts only, no time is meaningful"}
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")
    return 0 if all(x["agree_across_ranks"] and x["matches_formula"] and x["rc"] == 0 for x in modes) else 1


def collect(a, ps):
    ranks = []
    for q in ps:
        try:
            o, e = q.communicate(timeout=a.timeout)
        except subprocess.TimeoutExpired:
            for x in ps:
                x.kill()
            raise
        if q.returncode:
            for x in ps:
                x.kill()
            sys.exit(f"rank failed rc={q.returncode}: {e[-3000:]}")
        ranks.append(json.loads(o.strip().splitlines()[-1]))
    return ranks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("m", type=int)
    p.add_argument("N", type=int)
    p.add_argument("out", nargs="?")
    p.add_argument("--role", default="driver")
    p.add_argument("--timeout", type=float, default=900)
    p.add_argument("--krylov", action="store_true", help="count a flexible GMRES solve instead of single cycles")
    a = p.parse_args()
    if a.role == "rank":
        return rank_main_krylov(a.m) if a.krylov else rank_main(a.m)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(a.N),
               AMGD_ARENA_GB=os.environ.get("AMGD_ARENA_GB", str(max(8, 200 // a.N))))
    ps = [subprocess.Popen([sys.executable, "-u", __file__, str(a.m), str(a.N), "--role", "rank"]
                           + (["--krylov"] if a.krylov else []),
                           env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
          for r in range(a.N)]
    if a.krylov:
        return main_krylov(a, ps)
    ranks = collect(a, ps)
    modes = []
    for k, (name, _, halo) in enumerate(MODES):
        ms = [r["modes"][k] for r in ranks]
        lv = [list(v) for v in ms[0]["plan_levels"]]
        for other in ms[1:]:                       # entries of a distributed level: the ranks' rows together
            for l, v in enumerate(other["plan_levels"]):
                if not v[3]:
                    lv[l][2] += v[2]
        modes.append({"replication": name, "exchange": ms[0]["exchange"], "collectives": ms[0]["collectives"],
                      "bytes_sent_all_ranks": ms[0]["bytes_sent_all_ranks"],
                      "agree_across_ranks": all((x["collectives"], x["bytes_sent_all_ranks"]) ==
                                                (ms[0]["collectives"], ms[0]["bytes_sent_all_ranks"]) for x in ms),
                      "same_bits": all(x["same_bits"] for x in ms),
                      "levels_first_pos_nf_entries_replicated": lv})
    res = {"workload": f"3D 7-point Poisson {a.m}^3", "ranks": a.N, "levels": ranks[0]["levels"], "modes": modes,
           "transport": "host (gloo, N processes on one GPU): counts only, no time is meaningful"}
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")
    return 0 if all(x["same_bits"] and x["agree_across_ranks"] for x in modes) else 1


if __name__ == "__main__":
    sys.exit(main())
