"""Every operation of the row-partitioned layer (amgd_part.h: halos, the distributed transpose,
list syncs, eager exchanges, COO routing, gathers, kpos, the row and vector ops) called
directly, one pm_* call at a time, and compared bit for bit with the host restatement of the
one-GPU operation on the whole matrix -- on matrices and partitions no grid setup produces
(tests/part_cases.py: ragged cuts, ranks without rows, one owner, rectangular operands with
independent row and column partitions).  N processes share the test box's one GPU over the host
transport, with the collective guard on (tests/part_prim_worker.py); a failure names the
operation and the case, not a hierarchy array."""
import json
import os
import subprocess
import sys

import pytest

import part_cases as pc
from conftest import ROOT
from test_gpu_partition import _free_port

pytestmark = pytest.mark.gpu


# operation groups of part_prim_worker.py and the comparisons each makes per rank (per seed:
# induced 3, transpose 5, halo / spgemm 12, sub_mat 2, vector and diagonal ops 14; row ops and
# gathers 8, lists 8, route 2, kpos / zero_entries / coo_ones 3; 3 seeds; 9 eager calls)
EXCHANGES, ROWOPS = "induced,transpose,spgemm,sub_mat,vec", "rowops,lists,route,misc,eager"
CHECKS = {"": 180, EXCHANGES: 108, ROWOPS: 72}


def _spawn(size, kind, extra_env):
    """test_gpu_partition._spawn's launch (gloo rendezvous on a free port, the collective guard
    on, the same arena) with this file's worker"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(size),
               PART_CASE=kind, PYTHONPATH=ROOT, AMGD_COMM_CHECK="1",
               AMGD_ARENA_GB=os.environ.get("PART_ARENA_GB", "8"), **extra_env)
    return [subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "tests", "part_prim_worker.py")],
                             env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True) for r in range(size)]


def _run(size, kind, timeout=150, extra_env=None, groups=""):
    ps = _spawn(size, kind, dict(extra_env or {}, PART_GROUPS=groups))
    outs = []
    for p in ps:
        try:
            o, e = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in ps:
                q.kill()
            raise
        outs.append((p.returncode, o, e[-3000:]))
    res = []
    for r, (rc, o, e) in enumerate(outs):
        lines = o.strip().splitlines()
        try:
            d = json.loads(lines[-1])
        except (IndexError, ValueError):
            raise AssertionError("\n".join(f"--- rank {q} rc={c}\n{oo[-3000:]}\n{ee}" for q, (c, oo, ee) in
                                           enumerate(outs)))
        res.append(d)
    bad = [f"rank {d['rank']}: {b['op']} [{b['case']}]: {b['diff']}" for d in res for b in d["bad"]]
    assert not bad, f"{len(bad)} failing (op, case) on {size} ranks, {kind}:\n" + "\n".join(bad[:40])
    for (rc, o, e), d in zip(outs, res):
        assert d["leak_bytes"] == 0 and d["checks"] == CHECKS[groups] and d["calls"] > 0, d
        assert rc == 0, (d, e)
    print(size, kind, res[0]["checks"], "checks per rank")
    return res


# the 8-rank launches run the two operation groups in a launch each: all of them in one launch
# took 10.0 s (ragged) / 8.3 s (empty) against 4.3 s for the start-up-dominated
# test_partitioned_matches_reference_fixture[2-p7_12]; no case is left out
_LAUNCHES = [(n, k, g) for n, k in pc.LAUNCHES for g in (("",) if n < 8 else (EXCHANGES, ROWOPS))]


@pytest.mark.parametrize("size,kind,groups", _LAUNCHES,
                         ids=[f"{n}-{k}" + ("" if not g else "-exchanges" if g == EXCHANGES else "-rowops")
                              for n, k, g in _LAUNCHES])
def test_partitioned_primitives(size, kind, groups):
    """all operations for one (ranks, partition kind): 2, 3 and 4 ranks for every kind, 8 ranks
    for ragged cuts and for ranks without rows"""
    _run(size, kind, groups=groups)


def test_partitioned_primitives_poisoned():
    """4 ranks, ragged cuts, AMGD_POISON=1: every new array of doubles starts as NaN, so a read
    of a part no exchange or kernel wrote shows up in the comparison"""
    _run(4, "ragged", extra_env={"AMGD_POISON": "1"})


def test_partitioned_primitives_eager_slot_8():
    """4 ranks, ragged cuts, an 8-byte eager slot: every share of more than 8 bytes takes the
    exact second round (counted per call by the worker)"""
    _run(4, "ragged", extra_env={"PART_EAGER_SLOT": "8"})
