#!/usr/bin/env python3
"""The blocked Q-factor tiers alone (GPU box): one amgd_qfactor call per tier on the 27-point
20^3 matrix, supports of random size inside the tier (sorted random subsets of an index
window of 3 nz), about two residency rounds of them.  Run with AMGD_SGLOG=1: the library
prints each call's ms to stderr; this script prints the tier before each call and a SHA-256
of the packed factors after (the same under every AMGD_QF_CHAIN / AMGD_QF_PASS setting).

usage: AMGD_SGLOG=1 [AMGD_QF_CHAIN=0] [AMGD_QF_PASS=0] python tools/qf_tiers.py [reps]
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import omp_amg_amd as oa  # noqa: E402
from omp_amg_amd import abi, problems  # noqa: E402

M = 20
# tier: smallest size, largest size, supports
TIERS = {64: (33, 64, 12288), 128: (65, 128, 6144), 256: (129, 256, 3072), 512: (257, 400, 2048),
         1024: (513, 800, 512)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    Ai, Aj, Av = problems.poisson3d(M, 27)
    o = np.lexsort((Aj, Ai))
    aro, acol, aa = problems.coo_to_csr_np(np.asarray(Ai)[o], np.asarray(Aj)[o], np.asarray(Av)[o])
    A = abi.Csr(M ** 3, M ** 3, aro, acol, aa)
    oa.qf_split(0)
    for tier, (lo_n, hi_n, cnt) in TIERS.items():
        rng = np.random.default_rng(tier)
        sizes = rng.integers(lo_n, hi_n + 1, size=cnt)
        sup = []
        for nz in sizes:
            lo = int(rng.integers(0, M ** 3 - 3 * nz))
            sup.append(lo + np.sort(rng.choice(3 * nz, size=nz, replace=False)))
        ro = np.concatenate(([0], np.cumsum(sizes)))
        W = abi.Csr(cnt, M ** 3, ro, np.concatenate(sup).astype(np.int64), np.ones(int(ro[-1])))
        for rep in range(reps):
            print(f"# tier {tier} rep {rep}", file=sys.stderr, flush=True)
            X = oa.test_csr_op(5, W, A)
        sha = hashlib.sha256(np.ascontiguousarray(X.a).tobytes()).hexdigest()[:16]
        print(f"# tier {tier} sha {sha}", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
