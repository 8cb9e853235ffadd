"""omp_amg_amd -- MI355X-native AMG setup (hand-written HIP for gfx950) behind
the gslib C ABI of nicooff/omp_amg (amg_setup.h / crs.h).

Python here is only a ctypes mirror of that C ABI for tests and the bench:

  lib()                      -> ctypes.CDLL of omp_amg_amd/libomp_amg_amd.so (built in-tree)
  amg_setup(Ai, Aj, Av)      -> abi.Hierarchy     (reference amg_setup.h:5, host COO in)
  DeviceSetup                -> device-resident COO -> hierarchy in HBM (omp_amg_amd.h)
  stats()                    -> per-phase times of the last setup
  shard.*                    -> multi-GPU row sharding (RCCL / host transport / one-process sim)

The product path is the HIP library only: if it is missing or no GPU is
visible these functions raise -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libomp_amg_amd.so")
_lib = None


class AmgdStats(C.Structure):
    _fields_ = [("t_total_ms", C.c_double), ("t_build_ms", C.c_double),
                ("t_coarsen_ms", C.c_double), ("t_smoother_ms", C.c_double),
                ("t_interp_ms", C.c_double), ("t_rap_ms", C.c_double),
                ("t_copy_ms", C.c_double), ("rap_kernel_ms", C.c_double),
                ("rap_out_nnz", C.c_uint64), ("rap_bytes", C.c_uint64),
                ("rows0", C.c_uint64), ("nnz0", C.c_uint64),
                ("nlevels", C.c_uint32), ("ub_events", C.c_uint32),
                ("peak_bytes", C.c_size_t), ("spmv_kernel_ms", C.c_double),
                ("spmv_bytes", C.c_uint64), ("spmv_bytes_strict", C.c_uint64),
                ("spmv_launches", C.c_uint64), ("rap_launches", C.c_uint64),
                ("spmv_rw_ms", C.c_double * 3), ("spmv_rw_bytes_strict", C.c_uint64 * 3),
                ("spmv_rw_launches", C.c_uint64 * 3),
                ("ub_site", C.c_uint8 * 8), ("ub_level", C.c_uint8 * 8)]


class HCsr(C.Structure):
    """host CSR used by the kernel test hooks (amgd_testapi.c)"""
    _fields_ = [("rn", C.c_uint32), ("cn", C.c_uint32), ("nnz", C.c_uint64),
                ("ro", C.POINTER(C.c_uint64)), ("col", C.POINTER(C.c_uint32)),
                ("a", C.POINTER(C.c_double))]


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile the HIP library in-tree for gfx950 (make -C omp_amg_amd/csrc)."""
    args = ["make", "-C", os.path.join(HERE, "csrc"), f"-j{jobs}"]
    if force:
        subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "clean"], check=True)
    subprocess.run(args, check=True)
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run omp_amg_amd.build() (no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        abi.bind_setup(L)
        L.amgd_set_exact_dots.argtypes = [C.c_int]
        L.amgd_init.argtypes = [C.c_int]
        L.amgd_init.restype = C.c_int
        L.amgd_error.restype = C.c_char_p
        L.amgd_setup_device.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p), C.c_int]
        L.amgd_setup_device.restype = C.c_int
        L.amgd_hier_export.argtypes = [C.c_void_p, C.POINTER(abi.AmgSetupData)]
        L.amgd_hier_free.argtypes = [C.POINTER(C.c_void_p)]
        L.amgd_get_stats.argtypes = [C.POINTER(AmgdStats)]
        L.amgd_solve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.amgd_solve_device.restype = C.c_int
        L.amgd_solve_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                       C.POINTER(C.c_uint64)]
        L.amgd_solve_device_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int]
        L.amgd_solve_device_n.restype = C.c_int
        L.amgd_solve_n_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                         C.POINTER(C.c_uint64)]
        L.amgd_krylov_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.KrylovOpts),
                                         C.POINTER(abi.KrylovInfo), C.c_void_p, C.c_uint32]
        L.amgd_krylov_device.restype = C.c_int
        L.amgd_krylov_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.amgd_krylov_comm_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.amgd_test_kry_mdot_ranks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        L.amgd_test_kry_norm_ranks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                               C.c_void_p]
        L.amgd_test_kry_spmv_part.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.amgd_krylov_device_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                           C.POINTER(abi.KrylovOpts), C.POINTER(abi.KrylovInfo),
                                           C.POINTER(C.c_int), C.c_void_p, C.c_uint32]
        L.amgd_krylov_device_n.restype = C.c_int
        L.amgd_krylov_n_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_double)]
        L.amgd_test_kry_spmv_n.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_double, C.c_double, C.c_int, C.c_uint]
        L.amgd_test_kry_mdot_n.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p,
                                           C.c_void_p]
        L.amgd_test_kry_update_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                             C.c_void_p, C.c_void_p]
        L.amgd_test_kry_mdot.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        L.amgd_test_kry_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                           C.c_void_p]
        L.amgd_test_vc_level_n.argtypes = [C.POINTER(HCsr), C.POINTER(HCsr), C.POINTER(HCsr), C.c_void_p,
                                           C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_int]
        L.amgd_test_vc_restrict_n.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.amgd_test_vc_level.argtypes = [C.POINTER(HCsr), C.POINTER(HCsr), C.POINTER(HCsr), C.c_void_p,
                                         C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.amgd_test_vc_restrict.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_int]
        L.amgd_hier_rows.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.amgd_hier_rows.restype = C.c_int
        L.amgd_solve_comm_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.amgd_test_vc_restrict_map.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_uint32,
                                                C.c_void_p, C.c_int]
        L.amgd_test_vc_halo_xch.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_void_p]
        L.amgd_dev_alloc.argtypes = [C.c_size_t]
        L.amgd_dev_alloc.restype = C.c_void_p
        L.amgd_dev_free.argtypes = [C.c_void_p]
        L.amgd_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.amgd_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.amgd_test_csr.argtypes = [C.c_int, C.POINTER(HCsr), C.POINTER(HCsr), C.c_double,
                                    C.c_double, C.POINTER(HCsr)]
        L.amgd_test_spmv.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_double, C.c_void_p,
                                     C.c_double, C.c_void_p]
        L.amgd_test_spmv_f.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_double, C.c_void_p,
                                       C.c_double, C.c_void_p, C.c_void_p]
        L.amgd_test_spmv_rows.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.c_void_p]
        L.amgd_test_build.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(HCsr)]
        L.amgd_test_math.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.amgd_test_free.argtypes = [C.POINTER(HCsr)]
        L.amgd_test_dot.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.amgd_test_dot.restype = C.c_double
        L.amgd_test_lmop_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.amgd_test_qf_stats.argtypes = [C.POINTER(C.c_uint64)]
        L.amgd_test_spmv_shard_calls.restype = C.c_uint64
        L.amgd_test_route_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.amgd_comm_rccl_uid.argtypes = [C.c_char_p]
        L.amgd_comm_rccl_uid.restype = C.c_int
        L.amgd_comm_init_rccl.argtypes = [C.c_int, C.c_int, C.c_char_p]
        L.amgd_comm_init_rccl.restype = C.c_int
        L.amgd_comm_init_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.amgd_comm_init_host.restype = C.c_int
        L.amgd_comm_init_sim.argtypes = [C.c_int]
        L.amgd_comm_init_sim.restype = C.c_int
        L.amgd_comm_set_min_work.argtypes = [C.c_double]
        L.amgd_comm_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_double)]
        _lib = L
    return _lib


def init(device: int = 0) -> None:
    L = lib()
    if L.amgd_init(device) != 0:
        raise RuntimeError("omp_amg_amd: no usable HIP device: " + L.amgd_error().decode())


def amg_setup(Ai, Aj, Av, *, seed: int = 1) -> abi.Hierarchy:
    """Drop-in `amg_setup` (amg_setup.h:5) on host COO, through the C ABI."""
    init()
    return abi.run_setup(lib(), Ai, Aj, Av, seed=seed, quiet=False)


def stats() -> dict:
    st = AmgdStats()
    lib().amgd_get_stats(C.byref(st))
    out = {}
    for f, _ in AmgdStats._fields_:
        v = getattr(st, f)
        out[f] = list(v) if hasattr(v, "__len__") else v
    return out


class DeviceSetup:
    """COO resident in HBM -> hierarchy resident in HBM (omp_amg_amd.h)."""

    def __init__(self, Ai, Aj, Av):
        init()
        L = lib()
        self.nz = len(Av)
        Ai = np.ascontiguousarray(Ai, dtype=np.uint32)
        Aj = np.ascontiguousarray(Aj, dtype=np.uint32)
        Av = np.ascontiguousarray(Av, dtype=np.float64)
        self.di = L.amgd_dev_alloc(Ai.nbytes + 8)
        self.dj = L.amgd_dev_alloc(Aj.nbytes + 8)
        self.dv = L.amgd_dev_alloc(Av.nbytes + 8)
        L.amgd_dev_upload(self.di, Ai.ctypes.data, Ai.nbytes)
        L.amgd_dev_upload(self.dj, Aj.ctypes.data, Aj.nbytes)
        L.amgd_dev_upload(self.dv, Av.ctypes.data, Av.nbytes)
        self.h = C.c_void_p()

    def run(self, seed: int = 1, exact_dots: bool = True) -> dict:
        L = lib()
        L.amgd_set_exact_dots(1 if exact_dots else 0)
        if self.h:
            L.amgd_hier_free(C.byref(self.h))
        abi.srand(seed)
        rc = L.amgd_setup_device(self.nz, self.di, self.dj, self.dv, C.byref(self.h), 0)
        if rc != 0:
            raise RuntimeError("amgd_setup_device failed: " + L.amgd_error().decode())
        return stats()

    def export(self) -> abi.Hierarchy:
        L = lib()
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        raw = libc.malloc(C.sizeof(abi.AmgSetupData))
        C.memset(raw, 0, C.sizeof(abi.AmgSetupData))
        dp = C.cast(raw, C.POINTER(abi.AmgSetupData))
        L.amgd_hier_export(self.h, dp)
        h = abi.read_setup_data(dp.contents)
        L.free_data(C.pointer(dp))
        return h

    def vectors(self, n: int) -> None:
        """the device vectors db / dx of solve(), n doubles each (kept between solves)"""
        L = lib()
        if getattr(self, "_vec_n", 0) != n:
            for p in (getattr(self, "db", None), getattr(self, "dx", None)):
                if p:
                    L.amgd_dev_free(p)
            self.db = L.amgd_dev_alloc(n * 8 + 8)
            self.dx = L.amgd_dev_alloc(n * 8 + 8)
            self._vec_n = n

    def rows(self):
        """this rank's level-0 row range [r0, r1) of the kept hierarchy (one GPU: all rows)"""
        r0, r1 = C.c_uint32(), C.c_uint32()
        if lib().amgd_hier_rows(self.h, C.byref(r0), C.byref(r1)) != 0:
            raise RuntimeError("amgd_hier_rows failed")
        return int(r0.value), int(r1.value)

    def solve(self, b, remove_mean: bool = False, check: bool = True, complete: bool = False,
              partitioned: bool = False):
        """One V-cycle x = cycle(b) on the kept hierarchy (amgd_solve_device); b in level-0 row
        order.  check False: returns (rc, x) instead of raising on rc != 0.  partitioned (flag
        bit 2): the collective call on a partitioned hierarchy, which is refused (-3) without
        it: only the rank's own rows of b are read and of x written (the others come back NaN)
        unless complete (flag bit 1) asks for x whole on every rank."""
        L = lib()
        b = np.ascontiguousarray(b, dtype=np.float64)
        self.vectors(len(b))
        L.amgd_dev_upload(self.db, b.ctypes.data, b.nbytes)
        x = np.full(len(b), np.nan)
        L.amgd_dev_upload(self.dx, x.ctypes.data, x.nbytes)
        rc = L.amgd_solve_device(self.h, self.dx, self.db, (1 if remove_mean else 0) | (2 if complete else 0) | (4 if partitioned else 0))
        back = np.empty(len(b))
        if rc == 0:
            L.amgd_dev_download(x.ctypes.data, self.dx, b.nbytes)
        L.amgd_dev_download(back.ctypes.data, self.db, b.nbytes)
        self.b_after = back                       # db as the call left it (it must not change)
        if check and rc != 0:
            raise RuntimeError(f"amgd_solve_device failed rc={rc}: " + L.amgd_error().decode())
        return x if check else (rc, x)

    def solve_n(self, B, remove_mean: bool = False, ld=None, check: bool = True):
        """One V-cycle per column of B ((n0, nrhs), level-0 row order) in one call
        (amgd_solve_device_n): returns X (n0, nrhs), column j bit for bit solve(B[:, j]).
        ld: the device blocks' column stride (default n0); the padding rows of X are filled
        with NaN before the call and kept as `X_pad` after it, B's block as the call left it as
        `B_after`.  check False: returns (rc, X) instead of raising on rc != 0."""
        L = lib()
        B = np.asarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B[:, None]
        n0, nrhs = B.shape
        ld = n0 if ld is None else int(ld)
        rows = max(ld, n0)
        hb = np.zeros((max(nrhs, 1), rows))
        hb[:nrhs, :n0] = B.T
        hx = np.full((max(nrhs, 1), rows), np.nan)
        if getattr(self, "_nvec", 0) < hb.size:
            for p in (getattr(self, "dbn", None), getattr(self, "dxn", None)):
                if p:
                    L.amgd_dev_free(p)
            self.dbn = L.amgd_dev_alloc(hb.nbytes + 8)
            self.dxn = L.amgd_dev_alloc(hb.nbytes + 8)
            self._nvec = hb.size
        L.amgd_dev_upload(self.dbn, hb.ctypes.data, hb.nbytes)
        L.amgd_dev_upload(self.dxn, hx.ctypes.data, hx.nbytes)
        rc = L.amgd_solve_device_n(self.h, self.dxn, self.dbn, int(nrhs), ld, 1 if remove_mean else 0)
        back = np.empty_like(hb)
        if rc == 0:
            L.amgd_dev_download(hx.ctypes.data, self.dxn, hx.nbytes)
        L.amgd_dev_download(back.ctypes.data, self.dbn, hb.nbytes)
        self.B_after = back[:nrhs, :n0].T.copy()
        self.X_pad = hx[:nrhs, n0:].T.copy()
        if check and rc != 0:
            raise RuntimeError(f"amgd_solve_device_n failed rc={rc}: " + L.amgd_error().decode())
        X = hx[:nrhs, :n0].T.copy()
        return X if check else (rc, X)

    def krylov(self, b, rtol: float = 1e-8, atol: float = 0.0, restart: int = 0, maxit: int = 0,
               ordered: bool = False, x0=None, check: bool = True, partitioned: bool = False,
               complete: bool = False):
        """Solve A x = b on the kept hierarchy by restarted flexible GMRES with the V-cycle as
        the right preconditioner (amgd_krylov_device); b in level-0 row order.  restart / maxit
        0: the library's defaults (30 / 100).  ordered: every dot summed left to right (the
        verification path).  x0: the initial guess (flag bit 1).  Returns (x, info, hist): info
        a dict of amgd_krylov_info's fields and `rc`, hist the residual estimate after every
        inner iteration.  rc 0 converged, 1 maxit reached; check: raise on a negative rc
        (check False: x comes back NaN where the library did not write it).  partitioned (flag
        bit 2): the collective call on a partitioned hierarchy, refused (-3) without it: only
        the rank's own rows of b (and of x0) are read and of x written (without x0 the others
        come back NaN) unless complete (flag bit 3) asks for x whole on every rank."""
        L = lib()
        b = np.ascontiguousarray(b, dtype=np.float64)
        self.vectors(len(b))
        L.amgd_dev_upload(self.db, b.ctypes.data, b.nbytes)
        x = np.full(len(b), np.nan) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        L.amgd_dev_upload(self.dx, x.ctypes.data, x.nbytes)
        o = abi.KrylovOpts(rtol, atol, int(restart), int(maxit), (1 if ordered else 0) | (0 if x0 is None else 2)
                           | (4 if partitioned else 0) | (8 if complete else 0))
        info = abi.KrylovInfo()
        cap = int(maxit) if maxit else 100
        hist = np.full(cap, np.nan)
        rc = L.amgd_krylov_device(self.h, self.dx, self.db, C.byref(o), C.byref(info), hist.ctypes.data, cap)
        L.amgd_dev_sync()
        L.amgd_dev_download(x.ctypes.data, self.dx, b.nbytes)
        back = np.empty(len(b))
        L.amgd_dev_download(back.ctypes.data, self.db, b.nbytes)
        self.b_after = back
        if check and rc < 0:
            raise RuntimeError(f"amgd_krylov_device failed rc={rc}: " + L.amgd_error().decode())
        d = abi.krylov_info_dict(info, rc)
        return x, d, hist[:d["its"]].copy()

    def krylov_n(self, B, rtol: float = 1e-8, atol: float = 0.0, restart: int = 0, maxit: int = 0,
                 ordered: bool = False, X0=None, ld=None, check: bool = True):
        """Solve A X = B column by column in lock-step (amgd_krylov_device_n): B (n0, nrhs) in
        level-0 row order, the options of krylov(), X0 (n0, nrhs) the initial guesses (flag bit
        1).  Returns (X, infos, hists): column j of X, infos[j] (amgd_krylov_info's fields and
        the column's `rc`) and hists[j] are bit for bit what amgd_krylov_device gives on column j
        of the same device blocks.  ld: the blocks' column stride (default n0); the padding rows
        of X are filled with NaN before the call and kept as `X_pad` after it, B's block as the
        call left it as `B_after`, the call's own return value as `rc_n`.  A column the library
        did not write comes back NaN (its guess, if one was given).  check: raise when the call
        returns -1, -2 or -3."""
        L = lib()
        B = np.asarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B[:, None]
        n0, nrhs = B.shape
        ld = n0 if ld is None else int(ld)
        rows = max(ld, n0)
        hb = np.zeros((max(nrhs, 1), rows))
        hb[:nrhs, :n0] = B.T
        hx = np.full((max(nrhs, 1), rows), np.nan)
        if X0 is not None:
            hx[:nrhs, :n0] = np.asarray(X0, dtype=np.float64).T
        if getattr(self, "_nvec", 0) < hb.size:
            for p in (getattr(self, "dbn", None), getattr(self, "dxn", None)):
                if p:
                    L.amgd_dev_free(p)
            self.dbn = L.amgd_dev_alloc(hb.nbytes + 8)
            self.dxn = L.amgd_dev_alloc(hb.nbytes + 8)
            self._nvec = hb.size
        L.amgd_dev_upload(self.dbn, hb.ctypes.data, hb.nbytes)
        L.amgd_dev_upload(self.dxn, hx.ctypes.data, hx.nbytes)
        o = abi.KrylovOpts(rtol, atol, int(restart), int(maxit), (1 if ordered else 0) | (0 if X0 is None else 2))
        infos = (abi.KrylovInfo * max(nrhs, 1))()
        rcs = (C.c_int * max(nrhs, 1))(*([-1] * max(nrhs, 1)))
        cap = int(maxit) if maxit else 100
        hist = np.full((max(nrhs, 1), cap), np.nan)
        rc = L.amgd_krylov_device_n(self.h, self.dxn, self.dbn, int(nrhs), ld, C.byref(o), infos, rcs,
                                    hist.ctypes.data, cap)
        L.amgd_dev_sync()
        L.amgd_dev_download(hx.ctypes.data, self.dxn, hx.nbytes)
        back = np.empty_like(hb)
        L.amgd_dev_download(back.ctypes.data, self.dbn, hb.nbytes)
        self.B_after = back[:nrhs, :n0].T.copy()
        self.X_pad = hx[:nrhs, n0:].T.copy()
        self.rc_n = int(rc)
        if check and rc in (-1, -2, -3):
            raise RuntimeError(f"amgd_krylov_device_n failed rc={rc}: " + L.amgd_error().decode())
        ds = [abi.krylov_info_dict(infos[j], rcs[j] if rc not in (-1, -3) else rc) for j in range(nrhs)]
        hists = [hist[j, :ds[j]["its"]].copy() if rc not in (-1, -3) else hist[j, :0].copy() for j in range(nrhs)]
        return hx[:nrhs, :n0].T.copy(), ds, hists

    def krylov_at(self, j: int, ld: int, n0: int, rtol: float = 1e-8, atol: float = 0.0, restart: int = 0,
                  maxit: int = 0, ordered: bool = False, guess: bool = False):
        """amgd_krylov_device on column j of the device blocks the last krylov_n call left (B
        untouched by it; X holds that call's results, so with guess the caller uploads the
        guesses again through krylov_n_blocks): the single solver on the very pointers the
        multi-RHS call's contract names.  Returns (x, info, hist)."""
        L = lib()
        o = abi.KrylovOpts(rtol, atol, int(restart), int(maxit), (1 if ordered else 0) | (2 if guess else 0))
        info = abi.KrylovInfo()
        cap = int(maxit) if maxit else 100
        hist = np.full(cap, np.nan)
        rc = L.amgd_krylov_device(self.h, self.dxn + j * ld * 8, self.dbn + j * ld * 8, C.byref(o), C.byref(info),
                                  hist.ctypes.data, cap)
        L.amgd_dev_sync()
        x = np.empty(n0)
        L.amgd_dev_download(x.ctypes.data, self.dxn + j * ld * 8, x.nbytes)
        d = abi.krylov_info_dict(info, rc)
        return x, d, hist[:d["its"]].copy()

    def krylov_n_blocks(self, X, ld: int) -> None:
        """refill the device X block of the last krylov_n call: X (n0, nrhs), NaN in the padding"""
        X = np.asarray(X, dtype=np.float64)
        n0, nrhs = X.shape
        hx = np.full((nrhs, max(ld, n0)), np.nan)
        hx[:, :n0] = X.T
        lib().amgd_dev_upload(self.dxn, hx.ctypes.data, hx.nbytes)

    def close(self):
        L = lib()
        if self.h:
            L.amgd_hier_free(C.byref(self.h))
        for p in (getattr(self, "db", None), getattr(self, "dx", None), getattr(self, "dbn", None),
                  getattr(self, "dxn", None)):
            if p:
                L.amgd_dev_free(p)
        self.db = self.dx = self.dbn = self.dxn = None
        self._vec_n = 0
        self._nvec = 0
        for p in (self.di, self.dj, self.dv):
            if p:
                L.amgd_dev_free(p)
        self.di = self.dj = self.dv = None


# ---------------------------------------------------------------- test hooks
def _to_hcsr(ro, col, a, rn, cn):
    ro = np.ascontiguousarray(ro, dtype=np.uint64)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    a = np.ascontiguousarray(a, dtype=np.float64)
    h = HCsr(rn, cn, int(ro[-1]), ro.ctypes.data_as(C.POINTER(C.c_uint64)),
             col.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_double)))
    h._keep = (ro, col, a)
    return h


def _from_hcsr(h):
    rn, nz = h.rn, h.nnz
    ro = np.ctypeslib.as_array(h.ro, shape=(rn + 1,)).astype(np.int64)
    col = np.ctypeslib.as_array(h.col, shape=(max(nz, 1),))[:nz].astype(np.int64)
    a = np.ctypeslib.as_array(h.a, shape=(max(nz, 1),))[:nz].copy()
    out = abi.Csr(rn, h.cn, ro, col, a)
    lib().amgd_test_free(C.byref(h))
    return out


def test_csr_op(op: int, A: abi.Csr, B: abi.Csr | None = None, alpha=1.0, beta=1.0) -> abi.Csr:
    """op: 0 spgemm, 1 transpose, 2 mpm, 3 mxmpoint, 4 min_skel, 21 A back from its transpose
    (by the transpose's map, or the sort when a row is not strictly increasing), 23 the
    transpose with its values gathered through the map (kernel test hooks)."""
    init()
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    hb = _to_hcsr(B.row_off, B.col, B.a, B.rn, B.cn) if B is not None else None
    hx = HCsr()
    rc = lib().amgd_test_csr(op, C.byref(ha), C.byref(hb) if hb else None, alpha, beta, C.byref(hx))
    if rc != 0:
        raise RuntimeError(f"amgd_test_csr({op}) failed rc={rc}")
    return _from_hcsr(hx)


def test_csr_op3(op: int, A: abi.Csr, B: abi.Csr, B2: abi.Csr) -> abi.Csr:
    """op: 22 mxmpoint_sum(A, B, B2) = mxmpoint(A, mpm(1, B, 1, B2)) (kernel test hooks)."""
    init()
    L = lib()
    L.amgd_test_csr3.argtypes = [C.c_int, C.POINTER(HCsr), C.POINTER(HCsr), C.POINTER(HCsr),
                                 C.POINTER(HCsr)]
    hs = [_to_hcsr(M.row_off, M.col, M.a, M.rn, M.cn) for M in (A, B, B2)]
    hx = HCsr()
    rc = L.amgd_test_csr3(op, C.byref(hs[0]), C.byref(hs[1]), C.byref(hs[2]), C.byref(hx))
    if rc != 0:
        raise RuntimeError(f"amgd_test_csr3({op}) failed rc={rc}")
    return _from_hcsr(hx)


def test_spmv(A: abi.Csr, x, alpha=0.0, y=None, beta=1.0):
    init()
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    x = np.ascontiguousarray(x, dtype=np.float64)
    z = np.zeros(A.rn)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    lib().amgd_test_spmv(C.byref(ha), x.ctypes.data, alpha, None if yy is None else yy.ctypes.data,
                         beta, z.ctypes.data)
    return z


def test_spmv_f(A: abi.Csr, x=None, alpha=0.0, y=None, beta=1.0, f=None):
    """amgd_spmv with every option (x None: ordered row sums; f: u8 row mask)"""
    init()
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    ff = None if f is None else np.ascontiguousarray(f, dtype=np.uint8)
    z = np.zeros(A.rn)
    rc = lib().amgd_test_spmv_f(C.byref(ha), None if xx is None else xx.ctypes.data, alpha,
                                None if yy is None else yy.ctypes.data, beta,
                                None if ff is None else ff.ctypes.data, z.ctypes.data)
    if rc != 0:
        raise RuntimeError("amgd_test_spmv_f failed")
    return z


def test_spmv_tab(A: abi.Csr, x, alpha=0.0, y=None, beta=1.0, f=None, amx=False):
    """amgd_spmv on a pinned matrix: the gather-table kernel (k_spmv_tab).  Returns
    (z, amx or None, {builds, tiles, direct})"""
    init()
    L = lib()
    L.amgd_test_spmv_tab.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_double, C.c_void_p, C.c_double,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    ff = None if f is None else np.ascontiguousarray(f, dtype=np.uint8)
    z = np.zeros(A.rn)
    m = np.zeros(A.rn, dtype=np.uint64) if amx else None
    st = np.zeros(3, dtype=np.uint64)
    rc = L.amgd_test_spmv_tab(C.byref(ha), xx.ctypes.data, alpha, None if yy is None else yy.ctypes.data, beta,
                              None if ff is None else ff.ctypes.data, z.ctypes.data,
                              None if m is None else m.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_spmv_tab failed rc={rc}")
    return z, m, {"builds": int(st[0]), "tiles": int(st[1]), "direct": int(st[2])}


# ------------------------------------------------ the tuning switches (csrc/amgd_knob.h)
def knob(name: str, value=None) -> None:
    """override the switch `name` (its test-side name in the table) with `value`; None clears
    the override: the switch is then what its environment variable, else its default, says"""
    L = lib()
    L.amgd_test_knob.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    if L.amgd_test_knob(name.encode(), 0 if value is None else int(value), int(value is None)) != 0:
        raise KeyError(f"no switch named {name!r}")


def knob_get(name: str) -> tuple:
    """(effective value, source) of a switch; source 0 default, 1 environment, 2 override"""
    L = lib()
    L.amgd_test_knob_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    v, src = C.c_int64(), C.c_int()
    if L.amgd_test_knob_get(name.encode(), C.byref(v), C.byref(src)) != 0:
        raise KeyError(f"no switch named {name!r}")
    return int(v.value), int(src.value)


def knobs() -> list:
    """the whole table: name, environment variable (None: test-only), default, value, source"""
    L = lib()
    L.amgd_test_knob_info.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_int64)]
    out, i = [], 0
    name, env, dflt = C.c_char_p(), C.c_char_p(), C.c_int64()
    while L.amgd_test_knob_info(i, C.byref(name), C.byref(env), C.byref(dflt)) == 0:
        value, source = knob_get(name.value.decode())
        out.append({"name": name.value.decode(), "env": env.value.decode() if env.value else None,
                    "default": int(dflt.value), "value": value, "source": source})
        i += 1
    return out


def _nn(v):
    """a wrapper's negative argument means back to the environment / default"""
    return None if v < 0 else int(v)


def resolve_wave(on: int) -> None:
    """exact sums' (dots, long rows) resolution walk: 0 one 1024-thread block (the block walk,
    default), 1 one wavefront, -1 default / environment (AMGD_RESOLVE=wave: the wavefront)"""
    knob("resolve_wave", _nn(on))


def seg_split(on: int) -> None:
    """long-row exact sums: a chunk with one binade crossing resolved from its split record
    (1, default) or re-summed by the binade scan (0); -1: as AMGD_SEG_SPLIT says"""
    knob("seg_split", _nn(on))


def dot_split(on: int) -> None:
    """exact dots: a chunk with one binade crossing resolved from its split record (1, default)
    or re-summed by the binade scan (0); -1: as AMGD_DOT_SPLIT says (seg_split(0) turns off both)"""
    knob("dot_split", _nn(on))


def dot_spec_min(chunks: int) -> None:
    """exact dots: the length (in 4096-product chunks) from which the chunk speculation runs
    instead of one block's binade scan; -1: as AMGD_DOT_SPEC_MIN says (default 16)"""
    knob("dot_spec_min", _nn(chunks))


def spmv_tab(on: int) -> None:
    """gather tables for pinned long-row matrices: 1 on, 0 off (default), -1 default /
    environment (AMGD_MV_TAB)"""
    knob("spmv_tab", _nn(on))


def test_spmv_rows(A: abi.Csr, rows, x=None, z0=None):
    """amgd_spmv_rows: products (x None: ordered sums) of the listed rows only; the
    other entries of z keep z0"""
    init()
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    z = np.zeros(A.rn) if z0 is None else np.array(z0, dtype=np.float64)
    rc = lib().amgd_test_spmv_rows(C.byref(ha), rows.ctypes.data, len(rows),
                                   None if xx is None else xx.ctypes.data, z.ctypes.data)
    if rc != 0:
        raise RuntimeError("amgd_test_spmv_rows failed")
    return z


def spmv_sl_min(n: int) -> None:
    """row count from which whole-matrix and listed-row SpMVs with long rows run lane-per-row
    instead of wave-per-row (0: always, the default; -1: environment / default).  Same sums."""
    knob("spmv_sl_min", _nn(n))


def spmv_rw(rw: int) -> None:
    """rows per wavefront of the lane-per-row SpMV kernel: 4, 16 or 64 (-1: by row count).
    Same sums either way."""
    knob("spmv_rw", _nn(rw))


def spmv_rw_bounds(code: int) -> None:
    """row-count bounds of the lane SpMV's 16 / 64-row shapes as lo * 100 + hi (log2 of
    the row counts, e.g. 1622 = 2^16 / 2^22, the default; -1: default).  A/B only."""
    knob("spmv_rw_bounds", int(code) if code > 0 else None)


def qa_tile(t: int) -> None:
    """Q application of 33..512-point supports: U staged through LDS in 64 x t tiles
    (16 / 32) or the row-per-lane kernel (0); -1 back to the default.  Same sums."""
    knob("qa_tile", _nn(t))


def fs_amx(on: int) -> None:
    """find_support's selection after a full sweep: from the fused first maxima of the
    w = R' rs product (1, default) or by its own pass over the bad columns (0); -1 back to
    the default.  Same selections."""
    knob("fs_amx", _nn(on))


def d2h_poll(on: int) -> None:
    """small readbacks polled from host-coherent memory (1, default) or blocking copies
    (0); -1 back to the default.  A/B only: same results."""
    knob("d2h_poll", _nn(on))


def spmv_pair(on: int) -> None:
    """products with x through the paired-load lane kernel k_spmv_pair (1), the
    single-load k_spmv_pipe (0), or as AMGD_MV_PAIR says (-1).  Same sums either way."""
    knob("spmv_pair", _nn(on))


def test_build(Ai, Aj, Av) -> abi.Csr:
    init()
    Ai = np.ascontiguousarray(Ai, dtype=np.uint32)
    Aj = np.ascontiguousarray(Aj, dtype=np.uint32)
    Av = np.ascontiguousarray(Av, dtype=np.float64)
    hx = HCsr()
    lib().amgd_test_build(len(Av), Ai.ctypes.data, Aj.ctypes.data, Av.ctypes.data, C.byref(hx))
    return _from_hcsr(hx)


def test_math(op: int, a, b=None):
    init()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(a if b is None else b, dtype=np.float64)
    out = np.zeros_like(a)
    lib().amgd_test_math(op, len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out


def test_dot(mode: int, a, b=None, plain: bool = False, exact: bool = True) -> float:
    """exact (reference-order) dot through the library: mode 0 a.b, 1 a.a, 2 (a.*b).*b"""
    init()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(a if b is None else b, dtype=np.float64)
    return lib().amgd_test_dot(mode, len(a), a.ctypes.data, b.ctypes.data, int(plain), int(exact))


def lmop_mode(mode: int) -> None:
    """interp_lmop path: 0 = row-pull where order-exact (default), 1 = general key/sort walk"""
    knob("lmop_mode", _nn(mode))


def qf_sparse(mode: int) -> None:
    """huge-support Q factor: 0 dense cooperative, 1 sparse first (default),
    2 sparse with a capacity too small to finish (exercises the dense fallback)"""
    knob("qf_sparse", _nn(mode))


def qf_coop_lds(m: int) -> None:
    """dense cooperative huge-support factor: supports up to m points stage s1/s2/qk in
    LDS, larger ones read them from global memory (-1: default 8192)"""
    knob("qf_coop_lds", _nn(m))


def qa_huge(n: int) -> None:
    """Q application: supports above n points run the grid-wide kernels (-1: default 8192)"""
    knob("qa_huge", _nn(n))


def qf_split(on: int) -> None:
    """huge supports factored per connected component of A on the support (1, the
    default) or as one sequential factor (0); -1: back to the default / AMGD_QF_SPLIT"""
    knob("qf_split", _nn(on))


def mv_long(n: int) -> None:
    """listed-row products: rows past n entries take the block-per-row exact kernel
    (0: never; -1: default 4096 / AMGD_MV_LONG)"""
    knob("mv_long", _nn(n))


def fs_long(n: int) -> None:
    """find_support: rows / columns of R past n entries take the grid-wide expand and the
    block-per-column select (0: never; -1: default 4096 / AMGD_FS_LONG)"""
    knob("fs_long", _nn(n))


def qf_stats() -> dict:
    """huge supports factored sparse / sent to the dense kernel / split into components,
    since the last call"""
    out = (C.c_uint64 * 3)()
    lib().amgd_test_qf_stats(out)
    return {"sparse": int(out[0]), "fallback": int(out[1]), "split": int(out[2])}


ROUTES = ("spmv_pipe", "mv_long", "sg_tiny", "sg_kseq", "sg_wwin", "sg_wwin_sym", "sg_long",
          "cs_inc", "fs_inc", "sg_row", "mv_rw4", "qf_reuse", "lmop_wave", "mv_rw16", "mv_rw64",
          "qf_t512", "qf_t1024", "mv_pair", "fs_amx", "mv_tab", "sg_symreuse", "spat_inc", "sg_drsort",
          "skel_tr", "fs_sweep", "vc_thr", "vc_wave", "vc_comp", "vc_tail", "vc_halo", "vc_allg", "vc_repl",
          "qa_s16", "qa_s32", "qa_mid", "qa_blk", "qa_huge",
          "lmop_pull_thr", "lmop_pull_wave", "lmop_pull_blk", "lmop_qq_tile", "lmop_chunks",
          "vc_mr_thr", "vc_mr_wave", "vc_mr_single", "vc_mr_comp",
          "kry_it", "kry_mdot", "kry_odot",
          "kry_n_step", "kry_n_mixed", "kry_n_prod", "kry_n_single", "kry_n_comp",
          "kry_p_xch", "kry_p_comb")


def route_stats(reset: bool = True) -> dict:
    """how often each default kernel route ran since the last reset (amgd.h AMGD_R_*):
    lane SpMV, outlier-row SpMV, tiny / k-sequential / windowed / wide-symbolic /
    dense-slab / flat SpGEMM, incremental coarsening and find_support sweeps; fs_sweep counts
    every pass of find_support's loop; qa_*: Q application launches of the <= 16 / 17..32 /
    33..512-point / block kernels, qa_huge the supports on the grid-wide kernels; lmop_pull_*:
    row-pull launches per thread / wavefront / block, lmop_qq_tile the tiled QQ^t kernel,
    lmop_chunks the QQ^t chunks; vc_mr_thr / vc_mr_wave: multi-RHS V-cycle products by kernel
    family, vc_mr_single: columns of a multi-RHS call that took the single-vector cycle,
    vc_mr_comp: columns of one level's restriction / up-sweep run through the single-vector
    code because a matrix of the level has an outlier row; kry_it: inner iterations of the
    flexible GMRES, kry_mdot: its fused multi-dot launches, kry_odot: its ordered dots;
    kry_n_step: lock-step steps of krylov_n, kry_n_mixed: those whose active columns stood at two
    or more different inner indices, kry_n_prod: K-column level-0 product launches,
    kry_n_single: columns sent through the single-vector cycle or product as a group's leftover,
    kry_n_comp: per-column products of a matrix with an outlier row; kry_p_xch: exchanges before
    a level-0 product of the flexible GMRES on a partitioned hierarchy, kry_p_comb: its
    rank-order combines of the ranks' partial sums)"""
    out = (C.c_uint64 * len(ROUTES))()
    lib().amgd_test_route_stats(out, int(reset))
    return {k: int(out[i]) for i, k in enumerate(ROUTES)}


def lmop_stats(reset: bool = True) -> dict:
    """interp_lmop path counters since the last reset"""
    out = (C.c_uint64 * 5)()
    lib().amgd_test_lmop_stats(out, int(reset))
    return {"fast": out[0], "general": out[1], "dirty_prefix": out[2], "misses": out[3],
            "pruned": out[4]}


def lmop_prune(n: int) -> None:
    """general walk: supports of at least n points whose factor graph splits into
    components emit same-component contributions only (0: never; -1: default 4096 /
    AMGD_LMOP_PRUNE)"""
    knob("lmop_prune", _nn(n))


def spgemm_dr_sort(on: int) -> None:
    """SpGEMM rows past the hash bins' capacity by sorting their products (1, default) or by
    the one-block dense-slab kernel (0); -1: as AMGD_DR_SORT says"""
    knob("spgemm_dr_sort", _nn(on))


def spat_inc(on: int) -> None:
    """the constraint operator's pattern grown from the previous iteration's (1, default) or
    formed whole every iteration (0); -1: as AMGD_SPAT_INC says"""
    knob("spat_inc", _nn(on))


def skel_tr(on: int) -> None:
    """the interpolation loop's skeleton transposes (W0, the trial and final W, the Galerkin
    W') as permuted copies through the skeleton's own transpose map (1, default) or by the
    sort (0); -1: as AMGD_SKEL_TR says"""
    knob("skel_tr", _nn(on))


def fuse_arr(on: int) -> None:
    """W.*(Arhat + Ar) of the interpolation loop without forming the sum (1, default) or as
    mpm then mxmpoint (0); -1: as AMGD_FUSE_ARR says"""
    knob("fuse_arr", _nn(on))


def spat_stats() -> dict:
    out = (C.c_uint64 * 3)()
    lib().amgd_test_spat_stats(out)
    return {"incremental": out[0], "whole": out[1], "same": out[2]}


def spgemm_sym(mode: int) -> None:
    """the next one-GPU SpGEMM: 1 keeps its symbolic phase, 2 takes the kept one when the
    operand patterns match (else runs in full), -1 drops a kept state (tests)"""
    lib().amgd_test_spgemm_sym(int(mode))


def spgemm_sym_stats() -> dict:
    L = lib()
    k, r = C.c_uint64(), C.c_uint64()
    L.amgd_test_spgemm_sym_stats(C.byref(k), C.byref(r))
    return {"kept": k.value, "reused": r.value}


def spgemm_win(w: int) -> None:
    """wide output rows: 0 = LDS hash kernels only, 1024..16384 = every wide row through the
    wave-private windowed kernel (k_sg_wwin) whatever the column count, -1 = automatic"""
    knob("spgemm_win", _nn(w))


def qf_reuse(on: int) -> None:
    """Q factors of supports unchanged since the previous interpolation iteration: 1 copy
    (default), 0 refactor every support, -1 default / AMGD_QF_REUSE.  Same bits."""
    knob("qf_reuse", _nn(on))


def qf_chain(on: int) -> None:
    """blocked Q-factor tiers (33..1024 points): 1 the rows a block produces stay in
    registers for its later steps and the single-lane chains read LDS one batch ahead
    (default), 0 the kernel without either, -1 default / AMGD_QF_CHAIN.  Same bits."""
    knob("qf_chain", _nn(on))


def qf_pass(on: int) -> None:
    """blocked Q-factor kernel, 512- and 1024-point tiers only (the 64 / 128 / 256 tiers
    ignore it): 1 the two passes over the finished rows read their LDS operands four terms
    at a time and run whole batches without a per-term predicate (default), 0 the passes
    term by term, -1 default / AMGD_QF_PASS.  Same bits."""
    knob("qf_pass", _nn(on))


def qf_grid(n: int) -> None:
    """blocks per launch of the blocked Q-factor tiers; 0 (or -1): the default caps.  A
    small grid makes one block factor several supports in sequence."""
    knob("qf_grid", int(n) if n > 0 else None)


def lmop_wave(n: int) -> None:
    """interp_lmop general walk: chunks holding a support of >= n points replay sp_add's
    walk one wavefront per (c, k) with 64 columns searched at once (default 64), 0 one
    thread per (c, k) always, -1 default / AMGD_LMOP_WAVE.  Same landings."""
    knob("lmop_wave", _nn(n))


def sg_pattern(on: int) -> None:
    """constraint pattern W_skel*W_skel': 1 pattern-only product (default), 0 the full
    product (values discarded by interp_lmop), -1 default.  Same bits."""
    knob("sg_pattern", _nn(on))


def qa_small(on: int) -> None:
    """Q application: supports of <= 16 / 17..32 points on the lane-group kernels (1, default)
    or on the 33..512-point kernel with the rest (0); -1: as AMGD_QA_SMALL says.  Same sums."""
    knob("qa_small", _nn(on))


def lmop_qq_budget(nbytes: int) -> None:
    """interp_lmop row pull: bytes of QQ^t formed at a time, at least 1 MB (the coarse points
    are taken in chunks that fit); < 0: as AMGD_QQ_BUDGET_MB says (default 16 GB).  Same sums."""
    knob("lmop_qq_budget", _nn(nbytes))


def _hcsr_any(M):
    """an abi.Csr as HCsr, empty ones included"""
    h = _to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1),
                 M.rn, M.cn)
    h.nnz = int(M.row_off[-1])
    return h


def test_qapply(Wt: abi.Csr, A: abi.Csr, Bt: abi.Csr, u, lam):
    """The tail of interp on the device: the Q factors of Wt's rows (supports) on A, applied to
    Bt (one row per support), u (one per support) and lam (one per point).  Returns the
    nnz(Wt) values; an entry no kernel wrote is NaN."""
    init()
    L = lib()
    L.amgd_test_qapply.argtypes = [C.POINTER(HCsr), C.POINTER(HCsr), C.POINTER(HCsr), C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    hs = [_hcsr_any(M) for M in (Wt, A, Bt)]
    u = np.ascontiguousarray(u, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    assert len(u) == Wt.rn and len(lam) == Wt.cn
    out = np.zeros(int(Wt.row_off[-1]) + 1)
    rc = L.amgd_test_qapply(C.byref(hs[0]), C.byref(hs[1]), C.byref(hs[2]), u.ctypes.data,
                            lam.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_qapply failed rc={rc}")
    return out[:-1]


def test_lmop(S: abi.Csr, Wskel: abi.Csr, A: abi.Csr, u):
    """interp_lmop on the device: S's values on the caller's pattern from W_skel (values 1, 0
    on the dirty entries), A and u (one per column of W_skel), with the transpose, kpos and
    the Q factors formed as the setup forms them.  S's values start as NaN on the device."""
    init()
    L = lib()
    L.amgd_test_lmop.argtypes = [C.POINTER(HCsr), C.POINTER(HCsr), C.POINTER(HCsr), C.c_void_p,
                                 C.c_void_p]
    hs = [_hcsr_any(M) for M in (S, Wskel, A)]
    u = np.ascontiguousarray(u, dtype=np.float64)
    assert len(u) == Wskel.cn
    out = np.zeros(int(S.row_off[-1]) + 1)
    rc = L.amgd_test_lmop(C.byref(hs[0]), C.byref(hs[1]), C.byref(hs[2]), u.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_lmop failed rc={rc}")
    return out[:-1]


def lmop_small(n: int) -> None:
    """interp_lmop row pull: S rows of <= 32 entries one thread each (n > 0) or on the
    wavefront kernel (0); -1: back to the env (AMGD_LMOP_SMALL)"""
    knob("lmop_small", _nn(n))


def spgemm_flat(on: bool) -> None:
    """SpGEMM kernels: True = flat enumeration only, False = automatic (k-sequential for long B rows)"""
    knob("spgemm_flat", 1 if on else 0)


# ------------------------------------------------ row-partitioned primitives (test hooks)
class PmTargs(C.Structure):
    """pm_targs of amgd_testapi.c: the whole host operands, their splits, the op's vectors"""
    _fields_ = [("A", C.POINTER(HCsr)), ("B", C.POINTER(HCsr)),
                ("ars", C.c_void_p), ("acs", C.c_void_p), ("brs", C.c_void_p), ("bcs", C.c_void_p),
                ("a_nocol", C.c_int32), ("b_nocol", C.c_int32), ("iarg", C.c_int32), ("pad_", C.c_int32),
                ("alpha", C.c_double), ("beta", C.c_double),
                ("x", C.c_void_p), ("y", C.c_void_p),
                ("f", C.c_void_p), ("vr", C.c_void_p), ("vc", C.c_void_p),
                ("li", C.c_void_p), ("lj", C.c_void_p),
                ("nl", C.c_uint64), ("nl2", C.c_uint64),
                ("X", HCsr),
                ("z", C.c_void_p), ("z2", C.c_void_p),
                ("so_r", C.c_void_p), ("so_c", C.c_void_p),
                ("scalar", C.c_double)]


PM_OPS = {"transpose": 0, "spgemm": 1, "halo": 2, "sub_mat": 3, "mpm": 4, "mxmpoint": 5, "drop_zeros": 6,
          "rows_masked": 7, "diag_op": 8, "diag_op2": 9, "gather_full": 10, "gather_pattern": 11,
          "zero_entries": 12, "coo_ones": 13, "kpos": 14,
          "spmv": 20, "spmvt": 21, "colsum": 22, "diag": 23, "rowsum_sq_inv": 24, "fro": 25,
          "list_sync": 30, "list_sync2": 31, "list_rowsum": 32, "list_rowsum2": 33,
          "induced": 40, "route_coo": 41}


def _from_hcsr_opt(h):
    """a hook's X: col / a may be missing (values-only operands, gathered patterns)"""
    rn, nz = h.rn, h.nnz
    ro = np.ctypeslib.as_array(h.ro, shape=(rn + 1,)).astype(np.int64) if h.ro else None
    col = np.ctypeslib.as_array(h.col, shape=(max(nz, 1),))[:nz].astype(np.int64) if h.col else None
    a = np.ctypeslib.as_array(h.a, shape=(max(nz, 1),))[:nz].copy() if h.a else None
    out = abi.Csr(rn, h.cn, ro, col, a)
    lib().amgd_test_free(C.byref(h))
    return out


def test_pm(op: str, A=None, B=None, ars=None, acs=None, brs=None, bcs=None, a_nocol=False,
            b_nocol=False, iarg=0, alpha=0.0, beta=0.0, x=None, y=None, f=None, vr=None, vc=None,
            li=None, lj=None, z=None, z2=None):
    """One pm_* call of amgd_part.h on this rank's rows of the whole host operands (every rank
    of the partitioned communicator makes the same call).  A / B: abi.Csr; ars .. bcs: splits
    (size + 1 entries).  Returns {"X": local block, "z", "z2": whole vectors, "so_r", "so_c":
    induced splits, "scalar"} as the op fills them.  route_coo: X.a / X.col hold the received
    values / columns and "rows" the received rows."""
    init()
    L = lib()
    L.amgd_test_pm.argtypes = [C.c_int, C.POINTER(PmTargs)]
    keep = []

    def arr(v, dt):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=dt)
        if v.size == 0:                       # a valid address for an empty array
            v = np.zeros(1, dtype=dt)
        keep.append(v)
        return v.ctypes.data

    t = PmTargs()
    for name, M in (("A", A), ("B", B)):
        if M is not None:
            h = _to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1),
                         M.rn, M.cn)
            h.nnz = int(M.row_off[-1])
            keep.append(h)
            setattr(t, name, C.pointer(h))
    nsplit = len(ars if ars is not None else brs)
    t.ars, t.acs, t.brs, t.bcs = (arr(v, np.uint32) for v in (ars, acs, brs, bcs))
    t.a_nocol, t.b_nocol, t.iarg, t.alpha, t.beta = int(a_nocol), int(b_nocol), int(iarg), alpha, beta
    t.x, t.y = arr(x, np.float64), arr(y, np.float64)
    t.f, t.vr, t.vc = (arr(v, np.uint8) for v in (f, vr, vc))
    t.li, t.lj = arr(li, np.uint32), arr(lj, np.uint32)
    t.nl = 0 if li is None else len(li)
    t.nl2 = 0 if lj is None else len(lj)
    zo = None if z is None else np.array(z, dtype=np.float64)
    zo2 = None if z2 is None else np.array(z2, dtype=np.float64)
    t.z = None if zo is None else zo.ctypes.data
    t.z2 = None if zo2 is None else zo2.ctypes.data
    so_r, so_c = np.zeros(nsplit, dtype=np.uint32), np.zeros(nsplit, dtype=np.uint32)
    t.so_r, t.so_c = so_r.ctypes.data, so_c.ctypes.data
    rc = L.amgd_test_pm(PM_OPS[op], C.byref(t))
    if rc != 0:
        raise RuntimeError(f"amgd_test_pm({op}) failed rc={rc}")
    out = {"z": zo, "z2": zo2, "so_r": so_r.astype(np.int64), "so_c": so_c.astype(np.int64),
           "scalar": float(t.scalar), "X": None}
    if t.X.ro:
        if op == "route_coo":
            m = int(t.X.nnz)
            out["rows"] = np.ctypeslib.as_array(t.X.ro, shape=(max(m, 1),))[:m].astype(np.int64)
            t.X.rn = 0
            X = _from_hcsr_opt(t.X)
            X.row_off = None
            out["X"] = X
        else:
            out["X"] = _from_hcsr_opt(t.X)
    return out


def test_pm_eager(state: int, mine: bytes, user: int, size: int, cap: int):
    """pm_allgather_dyn with persistent call-site state `state` (0..3; < 0: a fresh one).
    Returns (concatenation bytes, len[size], users[size], total, the state's slot afterwards)"""
    init()
    L = lib()
    L.amgd_test_pm_eager.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    src = np.frombuffer(mine, dtype=np.uint8) if len(mine) else np.zeros(1, dtype=np.uint8)
    ln, us = np.zeros(size, dtype=np.uint64), np.zeros(size, dtype=np.uint64)
    tot, slot = C.c_uint64(), C.c_uint64()
    out = np.zeros(cap + 8, dtype=np.uint8)
    rc = L.amgd_test_pm_eager(state, src.ctypes.data, len(mine), user, ln.ctypes.data, us.ctypes.data,
                              C.byref(tot), out.ctypes.data, cap, C.byref(slot))
    if rc != 0:
        raise RuntimeError(f"amgd_test_pm_eager failed rc={rc}")
    return out[:tot.value].tobytes(), ln.astype(np.int64), us.astype(np.int64), int(tot.value), int(slot.value)


# ------------------------------------------------- find_support hooks (amgd_testapi.c)
FS_VARIANTS = {"plain": 0, "amx": 1, "windowed": 2}


def _ptr(a):
    return None if a is None else a.ctypes.data


def test_fs_select(variant: str, R: abi.Csr, rs, w, sumR, thr: float, pin: bool = True, c0: int = 0,
                   c1: int | None = None) -> dict:
    """One find_support selection sweep on R.  variant 'plain': amgd_fs_select; 'amx':
    amgd_spmv_amax(R', rs) then amgd_fs_select_amx ('amax' in the result is what amgd_spmv_amax
    returned; 0 means its kernel did not deliver the maxima and nothing was selected);
    'windowed': amgd_fs_select_ex on rows [c0, c1) of R' with perm NULL and resum 0, as the
    partitioned driver calls it.  pin: R and R' pinned as find_support pins them.  Returns
    sel (pairs (i, j) in device order), nremoved, amax, and R's values, R''s values (CSC
    order), rs and sumR after the call."""
    init()
    L = lib()
    L.amgd_test_fs_select.argtypes = [C.c_int, C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_double, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    hr = _to_hcsr(R.row_off, R.col, R.a, R.rn, R.cn)
    c1 = R.cn if c1 is None else c1
    rs = np.array(rs, dtype=np.float64)
    sumR = np.array(sumR, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    si = np.zeros(R.cn + 1, dtype=np.uint32)
    sj = np.zeros(R.cn + 1, dtype=np.uint32)
    out3 = np.zeros(3, dtype=np.uint32)
    nz = int(R.row_off[-1])
    Ra, Rta = np.zeros(nz + 1), np.zeros(nz + 1)
    rc = L.amgd_test_fs_select(FS_VARIANTS[variant], C.byref(hr), rs.ctypes.data, w.ctypes.data,
                               sumR.ctypes.data, float(thr), int(pin), int(c0), int(c1), si.ctypes.data,
                               sj.ctypes.data, out3.ctypes.data, Ra.ctypes.data, Rta.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_fs_select({variant}) failed rc={rc}")
    n = int(out3[0])
    return {"sel": np.stack([si[:n].astype(np.int64), sj[:n].astype(np.int64)], axis=1), "nsel": n,
            "nremoved": int(out3[1]), "amax": int(out3[2]), "Ra": Ra[:nz], "Rta": Rta[:nz], "rs": rs,
            "sumR": sumR}


def test_fs_expand(M: abi.Csr, rows, stamp, tag: int, cap: int, pin: bool = True):
    """amgd_fs_expand: the distinct columns of the listed rows of M whose stamp is not tag.
    Returns (count, out[:min(count, cap)], stamp after, the guard word behind out: 0xffffffff)"""
    init()
    L = lib()
    L.amgd_test_fs_expand.argtypes = [C.POINTER(HCsr), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    hm = _to_hcsr(M.row_off, M.col, M.a, M.rn, M.cn)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    st = np.array(stamp, dtype=np.uint32)
    out = np.zeros(cap + 1, dtype=np.uint32)
    res = np.zeros(2, dtype=np.uint32)
    rc = L.amgd_test_fs_expand(C.byref(hm), rows.ctypes.data, len(rows), st.ctypes.data, int(tag), int(cap),
                               int(pin), out.ctypes.data, res.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_fs_expand failed rc={rc}")
    return int(res[0]), out[:min(int(res[0]), cap)].astype(np.int64), st, int(res[1])


def test_fs_claim_ext(ids, stamp, tag: int, have, cap: int):
    """amgd_fs_claim_ext: ids claimed into out behind the entries `have` already there.
    Returns (count, out[:min(count, cap)], stamp after, guard word)"""
    init()
    L = lib()
    L.amgd_test_fs_claim_ext.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    st = np.array(stamp, dtype=np.uint32)
    out = np.zeros(cap + 1, dtype=np.uint32)
    out[:len(have)] = have
    res = np.zeros(2, dtype=np.uint32)
    rc = L.amgd_test_fs_claim_ext(ids.ctypes.data, len(ids), st.ctypes.data, len(st), int(tag), len(have),
                                  int(cap), out.ctypes.data, res.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_fs_claim_ext failed rc={rc}")
    return int(res[0]), out[:min(int(res[0]), cap)].astype(np.int64), st, int(res[1])


def test_fs_vec(op: str, a, b=None, thr: float = 0.0):
    """the reductions and vector kernel find_support's host decisions read: 'max_first' ->
    (value, index); 'max_first2' -> (value, index, max(b)); 'count_gt' -> (count, max);
    'vdiv_guard' -> a ./ b with 0 where b == 0"""
    init()
    L = lib()
    L.amgd_test_fs_vec.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                   C.c_void_p]
    code = {"max_first": 0, "max_first2": 1, "count_gt": 2, "vdiv_guard": 3}[op]
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    outd = np.zeros(max(len(a), 2) + 1)
    outu = np.zeros(2, dtype=np.uint64)
    rc = L.amgd_test_fs_vec(code, len(a), a.ctypes.data, _ptr(b), float(thr), outd.ctypes.data,
                            outu.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_fs_vec({op}) failed rc={rc}")
    if code == 0:
        return float(outd[0]), int(outu[0])
    if code == 1:
        return float(outd[0]), int(outu[0]), float(outd[1])
    if code == 2:
        return int(outu[0]), float(outd[0])
    return outd[:len(a)].copy()


def test_fs_mat(op: str, A: abi.Csr, x=None, y=None, rows=None, iarg: int = 0, z0=None):
    """'csc_gemv' -> A' x through the transpose's map (x None: column sums); 'list_rowsum' ->
    z0 with the ordered sums of the listed rows (iarg: long_rows); 'bad_rows' -> (mask, count);
    'skel_binarize' (iarg: mode) and 'scale_diag_match' (x = v, y = wuc) -> A's values after"""
    init()
    L = lib()
    L.amgd_test_fs_mat.argtypes = [C.c_int, C.POINTER(HCsr), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    code = {"csc_gemv": 0, "list_rowsum": 1, "bad_rows": 2, "skel_binarize": 3, "scale_diag_match": 4}[op]
    ha = _to_hcsr(A.row_off, A.col, A.a, A.rn, A.cn)
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    ll = np.ascontiguousarray([] if rows is None else rows, dtype=np.uint32)
    z = np.zeros(max(A.rn, A.cn) + 1) if z0 is None else np.array(z0, dtype=np.float64)
    mask = np.zeros(A.rn + 1, dtype=np.uint8)
    cnt = np.zeros(1, dtype=np.uint32)
    av = np.zeros(int(A.row_off[-1]) + 1)
    rc = L.amgd_test_fs_mat(code, C.byref(ha), _ptr(xx), _ptr(yy), ll.ctypes.data, len(ll), int(iarg),
                            z.ctypes.data, mask.ctypes.data, cnt.ctypes.data, av.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_fs_mat({op}) failed rc={rc}")
    if code == 0:
        return z[:A.cn].copy()
    if code == 1:
        return z
    if code == 2:
        return mask[:A.rn].copy(), int(cnt[0])
    return av[:int(A.row_off[-1])].copy()


def test_find_support(R: abi.Csr, goal: float, first=None):
    """the sweep loop of find_support (amgd_setup.c) on R.  first: (rs, w, tmp, w2), the first
    sweep's products handed in as interpolation hands them.  Returns (Sk, sweeps, first UB site
    or 0); the route counters fs_inc / fs_amx / fs_sweep count what it took."""
    init()
    L = lib()
    L.amgd_test_find_support.argtypes = [C.POINTER(HCsr), C.c_double, C.c_void_p, C.POINTER(HCsr),
                                         C.c_void_p]
    hr = _to_hcsr(R.row_off, R.col, R.a, R.rn, R.cn)
    fp = None
    if first is not None:
        keep = [np.ascontiguousarray(v, dtype=np.float64) for v in first]
        fp = (C.c_void_p * 4)(*[v.ctypes.data for v in keep])
    hx = HCsr()
    res = np.zeros(2, dtype=np.uint32)
    rc = L.amgd_test_find_support(C.byref(hr), float(goal), fp, C.byref(hx), res.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_find_support failed rc={rc}")
    return _from_hcsr(hx), int(res[0]), int(res[1])


# ------------------------------------------------------- V-cycle (amgd_vcycle.c)
def solve_stats() -> dict:
    """cycles run so far, their device-event time (ms) and the algorithmic bytes of one cycle
    of the hierarchy solved last"""
    c, ms, by = C.c_uint64(), C.c_double(), C.c_uint64()
    lib().amgd_solve_stats(C.byref(c), C.byref(ms), C.byref(by))
    return {"cycles": int(c.value), "ms": float(ms.value), "bytes": int(by.value)}


def krylov_stats() -> dict:
    """amgd_krylov_device calls and inner iterations so far and the calls' device-event time (ms)"""
    c, k, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    lib().amgd_krylov_stats(C.byref(c), C.byref(k), C.byref(ms))
    return {"calls": int(c.value), "its": int(k.value), "ms": float(ms.value)}


def krylov_comm_stats() -> dict:
    """collectives entered and bytes all ranks sent in the last krylov() call, the cycles' included
    (counts from the plan; the same on every rank)"""
    c, b = C.c_uint64(), C.c_uint64()
    lib().amgd_krylov_comm_stats(C.byref(c), C.byref(b))
    return {"collectives": int(c.value), "bytes": int(b.value)}


def _kry_own_block(V, ld):
    """a rank's rows of a basis (n, nb), n >= 0, as the column-major block of even stride ld"""
    V = np.asarray(V, dtype=np.float64)
    n, nb = V.shape
    ld = (n + 1) & ~1 if ld is None else int(ld)
    blk = np.full((nb, max(ld, 1)), np.nan)
    blk[:, :n] = V.T
    return np.ascontiguousarray(blk), n, nb, ld


def test_kry_mdot_ranks(V_own, w_own, ld=None):
    """the fused multi-dot of the partitioned solver on its own: this rank's rows V_own (n, nb)
    and w_own (n), n >= 0; every rank of the partitioned communicator makes the same call.
    Returns the nb sums v_t . w over all ranks: each rank's sums added in rank order"""
    init()
    blk, n, nb, ld = _kry_own_block(V_own, ld)
    w = np.ascontiguousarray(np.concatenate([np.asarray(w_own, dtype=np.float64), [np.nan]]))
    out = np.zeros(nb)
    if lib().amgd_test_kry_mdot_ranks(blk.ctypes.data, w.ctypes.data, n, ld, nb, out.ctypes.data) != 0:
        raise RuntimeError("amgd_test_kry_mdot_ranks failed")
    return out


def test_kry_norm_ranks(V_own, w_own, d, ld=None):
    """w = ((w - d_0 v_0) - d_1 v_1) - ... on this rank's rows, then the ranks' sums of the new
    w's squares added in rank order: returns (w_own, [the sum, its square root]); collective"""
    init()
    blk, n, nb, ld = _kry_own_block(V_own, ld)
    w = np.ascontiguousarray(np.concatenate([np.asarray(w_own, dtype=np.float64), [np.nan]]))
    d = np.ascontiguousarray(d, dtype=np.float64)
    nrm = np.zeros(2)
    if lib().amgd_test_kry_norm_ranks(blk.ctypes.data, w.ctypes.data, d.ctypes.data, n, ld, nb,
                                      nrm.ctypes.data) != 0:
        raise RuntimeError("amgd_test_kry_norm_ranks failed")
    return w[:n].copy(), nrm


def test_kry_spmv_part(M: abi.Csr, rsplit, vsplit, z):
    """the level-0 product of the partitioned solver on its own: this rank keeps rows
    rsplit[me]..rsplit[me+1] of the whole host matrix M, whose columns index the operand z owned
    by vsplit (valid on the own entries); the entries the rows read are fetched from their
    owners, then the rows' products are formed.  Returns (the own rows of M z, z after the
    exchange); collective"""
    init()
    h = _to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1), M.rn, M.cn)
    h.nnz = int(M.row_off[-1])
    rs = np.ascontiguousarray(rsplit, dtype=np.uint32)
    vs = np.ascontiguousarray(vsplit, dtype=np.uint32)
    me = int(lib().amgd_comm_rank())
    v = np.array(z, dtype=np.float64)
    out = np.full(int(rs[me + 1] - rs[me]) + 1, np.nan)
    rc = lib().amgd_test_kry_spmv_part(C.byref(h), rs.ctypes.data, vs.ctypes.data, v.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError("amgd_test_kry_spmv_part failed")
    return out[:-1].copy(), v


def krylov_n_stats() -> dict:
    """amgd_krylov_device_n calls, columns and lock-step steps so far and the calls' device-event
    time (ms)"""
    c, k, st, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    lib().amgd_krylov_n_stats(C.byref(c), C.byref(k), C.byref(st), C.byref(ms))
    return {"calls": int(c.value), "columns": int(k.value), "steps": int(st.value), "ms": float(ms.value)}


def kry_slots(n: int) -> None:
    """slots krylov_n may use (1..8; it never uses more than it has columns); -1: the default /
    AMGD_KRY_SLOTS.  Same bits."""
    knob("kry_slots", int(n) if n >= 1 else None)


def kry_family(family) -> None:
    """kernel family of krylov_n's K-column level-0 product: "auto" by the mean row length (long
    rows from 16), "short" / "long" forced, -1 the default / AMGD_KRY_MRHS_FAMILY.  Same bits."""
    knob("kry_family", None if family == -1 else VC_FAMILIES[family])


def test_kry_spmv_n(A: abi.Csr, X, alpha: float = 0.0, Y=None, beta: float = 1.0, family="auto", shift: int = 0):
    """the K-column level-0 product on its own: X (cn, K), Y (rn, K) or None, K = 2, 4 or 8;
    returns Z (rn, K) = alpha*Y + beta*(A X).  Every column is a device allocation of its own;
    bit j of shift starts column j one double into it (aligned to 8 bytes only).  A matrix with
    an outlier row goes column by column through the single-vector product (kry_n_comp)."""
    init()
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[1]
    xs = np.ascontiguousarray(X.T)
    ys = None if Y is None else np.ascontiguousarray(np.asarray(Y, dtype=np.float64).T)
    zs = np.full((K, A.rn), np.nan)
    hs = _hcsrs(A)
    rc = lib().amgd_test_kry_spmv_n(C.byref(hs[0]), xs.ctypes.data, None if ys is None else ys.ctypes.data,
                                    zs.ctypes.data, K, float(alpha), float(beta), VC_FAMILIES[family], int(shift))
    if rc != 0:
        raise RuntimeError("amgd_test_kry_spmv_n failed")
    return zs.T.copy()


def _kry_blocks(Vs, ws, ld):
    blks, nbs = [], []
    for V in Vs:
        blk, n, nb, ld_ = _kry_block(V, ld)
        blks.append(blk.ravel())
        nbs.append(nb)
    w = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64) for x in ws]))
    return np.concatenate(blks), w, n, ld_, np.ascontiguousarray(nbs, dtype=np.int32)


def test_kry_mdot_n(Vs, ws, ld=None):
    """test_kry_mdot for several columns in one launch: Vs[q] (n, nb_q), ws[q] (n); returns the
    list of the columns' dots"""
    init()
    blk, w, n, ld, nbs = _kry_blocks(Vs, ws, ld)
    out = np.zeros(int(nbs.sum()))
    if lib().amgd_test_kry_mdot_n(blk.ctypes.data, w.ctypes.data, n, ld, len(nbs), nbs.ctypes.data,
                                  out.ctypes.data) != 0:
        raise RuntimeError("amgd_test_kry_mdot_n failed")
    return np.split(out, np.cumsum(nbs)[:-1])


def test_kry_update_n(Vs, ws, ds, ld=None, norm: bool = False):
    """test_kry_update for several columns in one launch; returns the list of the new w (norm:
    of (w, [sum of squares, root]))"""
    init()
    blk, w, n, ld, nbs = _kry_blocks(Vs, ws, ld)
    d = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in ds]))
    nrm = np.zeros((len(nbs), 2))
    if lib().amgd_test_kry_update_n(blk.ctypes.data, w.ctypes.data, d.ctypes.data, n, ld, len(nbs),
                                    nbs.ctypes.data, nrm.ctypes.data if norm else None) != 0:
        raise RuntimeError("amgd_test_kry_update_n failed")
    return [(w[q].copy(), nrm[q].copy()) for q in range(len(nbs))] if norm else [w[q].copy() for q in range(len(nbs))]


def kry_tile() -> int:
    """basis vectors per workgroup row of the fused multi-dot (amgd_krylov.hip)"""
    return int(lib().amgd_test_kry_tile())


def _kry_block(V, ld):
    """(n, nb) -> the column-major host block with stride ld, NaN in the padding"""
    V = np.asarray(V, dtype=np.float64)
    n, nb = V.shape
    ld = n if ld is None else int(ld)
    blk = np.full((nb, ld), np.nan)
    blk[:, :n] = V.T
    return np.ascontiguousarray(blk), n, nb, ld


def test_kry_mdot(V, w, ld=None):
    """the fused multi-dot on a basis block V (n, nb) with column stride ld (default n): the nb
    sums v_t . w"""
    init()
    blk, n, nb, ld = _kry_block(V, ld)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros(nb)
    if lib().amgd_test_kry_mdot(blk.ctypes.data, w.ctypes.data, n, ld, nb, out.ctypes.data) != 0:
        raise RuntimeError("amgd_test_kry_mdot failed")
    return out


def test_kry_update(V, w, d, ld=None, norm: bool = False):
    """w = ((w - d_0 v_0) - d_1 v_1) - ... by the update kernel; norm: returns (w, [sum of the
    new w's squares, its square root]) from the kernel's own partials"""
    init()
    blk, n, nb, ld = _kry_block(V, ld)
    w = np.array(w, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    nrm = np.zeros(2)
    if lib().amgd_test_kry_update(blk.ctypes.data, w.ctypes.data, d.ctypes.data, n, ld, nb,
                                  nrm.ctypes.data if norm else None) != 0:
        raise RuntimeError("amgd_test_kry_update failed")
    return (w, nrm) if norm else w


def solve_n_stats() -> dict:
    """multi-RHS calls (solve_n) and columns so far, the calls' device-event time (ms) and the
    algorithmic bytes of the last call (matrices once per group, those of a level that fell back
    column by column once per column; vectors per column)"""
    c, k, ms, by = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_uint64()
    lib().amgd_solve_n_stats(C.byref(c), C.byref(k), C.byref(ms), C.byref(by))
    return {"calls": int(c.value), "columns": int(k.value), "ms": float(ms.value), "bytes": int(by.value)}


def vc_mrhs_k(sizes) -> None:
    """group sizes solve_n may use: an iterable out of {2, 4, 8} (empty: every column through
    the single-vector cycle), or -1 for the default / AMGD_VC_MRHS_K.  Same bits."""
    if isinstance(sizes, int) and sizes < 0:
        knob("vc_mrhs_k", None)
        return
    mask = 0
    for k in sizes:
        if int(k) not in (2, 4, 8):
            raise ValueError("group sizes are 2, 4 and 8")
        mask |= int(k)
    knob("vc_mrhs_k", mask)


def vc_row_max(n: int) -> None:
    """solve plans and level hooks from now on treat rows of more than n entries as outlier rows
    (composed single-vector products; column by column in solve_n); 0: the default, 4 096"""
    knob("vc_row_max", int(n) if n > 0 else None)


VC_FAMILIES = {"auto": 0, "short": 1, "long": 2}


def vc_mrhs_family(family) -> None:
    """kernel family of solve_n's products: "auto" by row shape (short-row kernels below a mean
    row of 16, long-row kernels from there), "short" / "long" forced, -1 the default /
    AMGD_VC_MRHS_FAMILY.  Same bits."""
    knob("vc_mrhs_family", None if family == -1 else VC_FAMILIES[family])


def _hcsrs(*Ms):
    hs = [_to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1),
                   M.rn, M.cn) for M in Ms]
    for h, M in zip(hs, Ms):
        h.nnz = int(M.row_off[-1])
    return hs


def test_vc_level_n(Af: abi.Csr, W: abi.Csr, AfP: abi.Csr, D, m: int, rho: float, BF, XC, family="auto"):
    """test_vc_level on K = 2, 4 or 8 columns through the K-column kernels: BF (nf, K), XC
    (nc, K); family: the kernels by row shape, or the short-row / long-row family forced.
    Returns (XF, BF, C), each (nf, K)."""
    init()
    hs = _hcsrs(Af, W, AfP)
    nf, nc = W.rn, W.cn
    BF = np.asarray(BF, dtype=np.float64).reshape(nf, -1)
    XC = np.asarray(XC, dtype=np.float64).reshape(nc, -1)
    K = BF.shape[1]
    D = np.ascontiguousarray(D, dtype=np.float64)
    X = np.full((K, nf + nc), np.nan)               # xf is written, never read first
    X[:, nf:] = XC.T
    B = np.array(BF.T, order="C")               # a copy: the hook writes into it
    Cbuf = np.zeros(K * max(nf, 1))
    rc = lib().amgd_test_vc_level_n(C.byref(hs[0]), C.byref(hs[1]), C.byref(hs[2]), D.ctypes.data, int(m),
                                    float(rho), X.ctypes.data, B.ctypes.data, Cbuf.ctypes.data, int(K),
                                    VC_FAMILIES[family])
    if rc != 0:
        raise RuntimeError(f"amgd_test_vc_level_n(K={K}, {family}) failed rc={rc}")
    Cc = Cbuf[:K * nf].reshape(K, nf)
    return X[:, :nf].T.copy(), B.T.copy(), Cc.T.copy()


def test_vc_restrict_n(W: abi.Csr, BF, BC, family="auto"):
    """BC + W' BF on K = 2, 4 or 8 columns: BF (nf, K), BC (nc, K); returns (nc, K)"""
    init()
    (h,) = _hcsrs(W)
    BF = np.asarray(BF, dtype=np.float64).reshape(W.rn, -1)
    BC = np.asarray(BC, dtype=np.float64).reshape(W.cn, -1)
    K = BF.shape[1]
    F = np.ascontiguousarray(BF.T)
    out = np.array(BC.T, order="C")             # a copy: the hook writes into it
    rc = lib().amgd_test_vc_restrict_n(C.byref(h), F.ctypes.data, out.ctypes.data, int(K), VC_FAMILIES[family])
    if rc != 0:
        raise RuntimeError(f"amgd_test_vc_restrict_n(K={K}, {family}) failed rc={rc}")
    return out.T.copy()


def vc_fused(on: int) -> None:
    """V-cycle kernels: 1 the fused kernels of amgd_solve.hip where a shape has one (default),
    0 composed from the setup's kernels, -1 as AMGD_VC_FUSED says.  Same bits."""
    knob("vc_fused", _nn(on))


def vc_coop(on: int) -> None:
    """long-row shapes of the fused path: 1 the cooperative kernels, 0 composed, -1 default /
    AMGD_VC_COOP.  Same bits."""
    knob("vc_coop", _nn(on))


def vc_rw(rw: int) -> None:
    """cooperative V-cycle kernels: rows per wavefront 4, 16 or 64 (0: by row count).  Same bits."""
    knob("vc_rw", int(rw) if rw in (4, 16, 64) else None)


def vc_tail(rows: int) -> None:
    """the one-workgroup coarse tail: the deepest levels of at most `rows` positions together
    (0 off, at most 1024, -1: default 1024 / AMGD_VC_TAIL=0 off).  Same bits."""
    knob("vc_tail", _nn(rows))


def vc_halo(on: int) -> None:
    """partitioned V-cycle exchanges: 1 halo lists (pack, alltoallv, unpack; default), 0 an
    allgatherv of the whole F segment, -1 as AMGD_VC_HALO says.  Same bits."""
    knob("vc_halo", _nn(on))


def vc_repl(rows: int) -> None:
    """partitioned V-cycle: levels whose slice has at most `rows` positions run replicated on
    every rank (0: the bottom level only; -1: default / AMGD_VC_REPL_ROWS).  Same bits."""
    knob("vc_repl", _nn(rows))


def solve_comm_stats() -> dict:
    """collectives entered and bytes all ranks sent in the last solve (counts from the plan)"""
    c, b = C.c_uint64(), C.c_uint64()
    lib().amgd_solve_comm_stats(C.byref(c), C.byref(b))
    return {"collectives": int(c.value), "bytes": int(b.value)}


VC_MAP_MODES = {"composed": 0, "thr": 1, "coop": 2}


def test_vc_restrict_map(Wt: abi.Csr, bF, b, cmap, mode="thr"):
    """b[cmap[c]] += row c of Wt times bF (the partitioned cycle's restriction on a rank's own
    C rows) on host operands; returns b"""
    init()
    h = _to_hcsr(Wt.row_off, Wt.col if len(Wt.col) else np.zeros(1), Wt.a if len(Wt.a) else np.zeros(1),
                 Wt.rn, Wt.cn)
    h.nnz = int(Wt.row_off[-1])
    bF = np.ascontiguousarray(bF, dtype=np.float64)
    out = np.array(b, dtype=np.float64)
    cm = np.ascontiguousarray(cmap, dtype=np.uint32)
    rc = lib().amgd_test_vc_restrict_map(C.byref(h), bF.ctypes.data, out.ctypes.data, len(out),
                                         cm.ctypes.data, VC_MAP_MODES[mode])
    if rc != 0:
        raise RuntimeError("amgd_test_vc_restrict_map failed")
    return out


def test_vc_halo_xch(M: abi.Csr, rsplit, vsplit, v):
    """one halo exchange of the partitioned cycle on its own: this rank keeps rows
    rsplit[me]..rsplit[me+1] of the whole host matrix M, whose columns index the vector v owned by
    vsplit; returns v with every entry the rows reference fetched from its owner (every rank of the
    partitioned communicator makes the same call)"""
    init()
    h = _to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1), M.rn, M.cn)
    h.nnz = int(M.row_off[-1])
    rs = np.ascontiguousarray(rsplit, dtype=np.uint32)
    vs = np.ascontiguousarray(vsplit, dtype=np.uint32)
    out = np.array(v, dtype=np.float64)
    rc = lib().amgd_test_vc_halo_xch(C.byref(h), rs.ctypes.data, vs.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError("amgd_test_vc_halo_xch failed")
    return out


VC_MODES = {"composed": 0, "fused": 1, "tail": 2}


def test_vc_level(Af: abi.Csr, W: abi.Csr, AfP: abi.Csr, D, m: int, rho: float, bf, xc, mode="fused"):
    """one level's up-sweep (xf = W xc, bf -= AfP xc, m Chebyshev steps, xf += c) on host
    operands; W / AfP columns index xc.  Returns (xf, bf, c)."""
    init()
    hs = [_to_hcsr(M.row_off, M.col if len(M.col) else np.zeros(1), M.a if len(M.a) else np.zeros(1),
                   M.rn, M.cn) for M in (Af, W, AfP)]
    for h, M in zip(hs, (Af, W, AfP)):
        h.nnz = int(M.row_off[-1])
    nf = W.rn
    D = np.ascontiguousarray(D, dtype=np.float64)
    bf = np.ascontiguousarray(bf, dtype=np.float64)
    xc = np.ascontiguousarray(xc, dtype=np.float64)
    out = [np.zeros(max(nf, 1)) for _ in range(3)]
    rc = lib().amgd_test_vc_level(C.byref(hs[0]), C.byref(hs[1]), C.byref(hs[2]), D.ctypes.data, int(m),
                                  float(rho), bf.ctypes.data, xc.ctypes.data, VC_MODES[mode],
                                  out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    if rc != 0:
        raise RuntimeError(f"amgd_test_vc_level({mode}) failed rc={rc}")
    return tuple(o[:nf] for o in out)


def test_vc_restrict(W: abi.Csr, bF, bC, fused: bool = True):
    """bC + W' bF (one level's restriction) on host operands"""
    init()
    h = _to_hcsr(W.row_off, W.col if len(W.col) else np.zeros(1), W.a if len(W.a) else np.zeros(1), W.rn, W.cn)
    h.nnz = int(W.row_off[-1])
    bF = np.ascontiguousarray(bF, dtype=np.float64)
    out = np.array(bC, dtype=np.float64)
    rc = lib().amgd_test_vc_restrict(C.byref(h), bF.ctypes.data, out.ctypes.data, int(fused))
    if rc != 0:
        raise RuntimeError("amgd_test_vc_restrict failed")
    return out
