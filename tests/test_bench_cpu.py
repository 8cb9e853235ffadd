"""bench.py's command line and its --dump-outputs writer, without a GPU: the oracle's
amg_setup fills the struct amg_setup_data that amgd_hier_export fills on the device path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench
from omp_amg_amd import abi, problems


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, check=True).stdout
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out, opt


@pytest.fixture(scope="module")
def setup_case(oracle_lib):
    Ai, Aj, Av = problems.poisson3d(9)
    return (Ai, Aj, Av), abi.run_setup(oracle_lib, Ai, Aj, Av)


class _OracleExport:
    """stands in for the HIP library in dump_outputs: same struct out, same free_data"""

    def __init__(self, lib, coo):
        self.lib, self.coo = lib, coo

    def amgd_hier_export(self, h, dp):
        Ai, Aj, Av = self.coo
        ai = np.ascontiguousarray(Ai, dtype=np.uint64)
        aj = np.ascontiguousarray(Aj, dtype=np.uint64)
        u = C.POINTER(abi.amg_uint)
        abi.srand(1)
        with abi.quiet_stdout():
            self.lib.amg_setup(len(Av), ai.ctypes.data_as(u), aj.ctypes.data_as(u),
                               Av.ctypes.data_as(C.POINTER(C.c_double)), dp)
        return 0

    def free_data(self, pp):
        self.lib.free_data(pp)


class _NoHandle:
    h = None


def _expected(h):
    out = {"setup": np.array([h.nlevels, h.nullspace, h.tolc, h.gamma]), "id": h.id}
    lv = np.zeros((h.nlevels, 6))
    for l, lev in enumerate(h.levels):
        mats = {"A": lev.A}
        lv[l, :2] = lev.n, lev.nnz
        if lev.W is not None:
            lv[l, 2:] = lev.nnzf, lev.nnzfp, lev.m, lev.rho
            mats.update(Af=lev.Af, W=lev.W, AfP=lev.AfP)
            for f in ("C", "F", "D", "idc", "idf"):
                out[f"L{l}_{f}"] = getattr(lev, f)
        for k, m in mats.items():
            out[f"L{l}_{k}_ro"], out[f"L{l}_{k}_col"], out[f"L{l}_{k}_a"] = m.row_off, m.col, m.a
    out["levels"] = lv.ravel()
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


@pytest.mark.parametrize("share", [None, 100], ids=["whole", "sampled"])
def test_dump_outputs_is_the_exported_hierarchy(oracle_lib, setup_case, tmp_path, monkeypatch, share):
    coo, ref = setup_case
    import omp_amg_amd as oa
    monkeypatch.setattr(oa, "lib", lambda: _OracleExport(oracle_lib, coo))
    want = _expected(ref)
    if share is not None:                       # every array's share: `share` entries
        monkeypatch.setattr(bench, "DUMP_BYTES", share * 8 * len(want))
    cap = bench.DUMP_BYTES // 8 // len(want)
    total = bench.dump_outputs(_NoHandle(), str(tmp_path))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == sorted(want)
    assert total == sum(v.nbytes for v in got.values()) <= bench.DUMP_BYTES
    sampled = 0
    for k, w in want.items():
        assert got[k].dtype == np.float64, k
        if len(w) > cap:
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, len(w), size=cap))
            w = w[idx]
            sampled += 1
        assert np.array_equal(got[k].view(np.uint64), w.view(np.uint64)), k
    assert (sampled > 0) == (share is not None)
