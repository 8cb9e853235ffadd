"""The switch table (omp_amg_amd/csrc/amgd_knob.h) without a GPU: defaults, the environment,
overrides and re-reads through the library's test hooks; the Python wrappers on top of it; the
table against INTEGRATION.md and against the sources; the table alone under host sanitizers."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

import omp_amg_amd as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omp_amg_amd", "csrc")
# variables the library reads that are not switches (the head comment of amgd_knob.h names them)
NOT_SWITCHES = {"AMGD_DUMP", "AMGD_TRACE_MAX_IT", "AMGD_TRACE_MAX_S"}


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(oa.LIB_PATH):
        oa.build()


@pytest.fixture
def clean_env(monkeypatch):
    """no switch variable set, no override; the environment is read again before and after"""
    for k in list(os.environ):
        if k.startswith("AMGD_"):
            monkeypatch.delenv(k)
    for e in oa.knobs():
        oa.knob(e["name"], None)
    reread()
    yield monkeypatch
    monkeypatch.undo()
    for e in oa.knobs():
        oa.knob(e["name"], None)
    reread()


def reread():
    oa.lib().amgd_test_knobs_reread()


def test_defaults_and_names(clean_env):
    table = oa.knobs()
    assert len(table) > 60
    names = [e["name"] for e in table]
    assert len(set(names)) == len(names)
    envs = [e["env"] for e in table if e["env"]]
    assert len(set(envs)) == len(envs) and all(re.fullmatch(r"AMGD_[A-Z0-9_]+", v) for v in envs)
    for e in table:
        assert oa.knob_get(e["name"]) == (e["default"], 0), e
    for test_only in ("qf_grid", "qf_coop_lds", "qa_huge", "spmv_rw_bounds", "vc_row_max", "vc_rw", "sg_pattern"):
        assert next(e for e in table if e["name"] == test_only)["env"] is None


@pytest.mark.parametrize("name,env,text,value,text2,value2", [
    ("qf_chain", "AMGD_QF_CHAIN", "0", 0, "3", 3),                       # a number
    ("cs_min_rows", "AMGD_CS_MIN_ROWS", "12345678901", 12345678901, "0", 0),
    ("resolve_wave", "AMGD_RESOLVE", "wave", 1, "block", 0),             # parse functions
    ("vc_mrhs_k", "AMGD_VC_MRHS_K", "4,2", 6, "8", 8),
    ("hbm_cap", "AMGD_HBM_CAP_GB", "1.5", 3 << 29, "2", 2 << 30),
    ("sglog", "AMGD_SGLOG", "1", 1, "0", 0),                             # a log flag: 0 is off
])
def test_environment_override_clear_reread(clean_env, name, env, text, value, text2, value2):
    dflt = oa.knob_get(name)[0]
    clean_env.setenv(env, text)
    assert oa.knob_get(name) == (dflt, 0)            # not before the next read
    reread()
    assert oa.knob_get(name) == (value, 1)
    oa.knob(name, 41)                                 # an override beats the environment
    assert oa.knob_get(name) == (41, 2)
    clean_env.setenv(env, text2)
    reread()
    assert oa.knob_get(name) == (41, 2)
    oa.knob(name, None)                               # a clear returns to it, as last read
    assert oa.knob_get(name) == (value2, 1)
    clean_env.setenv(env, "")                         # empty means unset
    reread()
    assert oa.knob_get(name) == (dflt, 0)
    clean_env.delenv(env)
    reread()
    assert oa.knob_get(name) == (dflt, 0)


def test_unknown_name():
    L = oa.lib()
    L.amgd_test_knob.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    L.amgd_test_knob_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    v, s = C.c_int64(), C.c_int()
    assert L.amgd_test_knob(b"no_such_switch", 1, 0) == -1
    assert L.amgd_test_knob(b"no_such_switch", 0, 1) == -1
    assert L.amgd_test_knob_get(b"AMGD_QF_CHAIN", C.byref(v), C.byref(s)) == -1   # names, not variables
    with pytest.raises(KeyError):
        oa.knob("no_such_switch", 1)
    with pytest.raises(KeyError):
        oa.knob_get("")


# every public function of omp_amg_amd/__init__.py at the parent of the commit that added the table
PARENT_API = """build lib init amg_setup stats test_csr_op test_csr_op3 test_spmv test_spmv_f test_spmv_tab
resolve_wave seg_split dot_split dot_spec_min spmv_tab test_spmv_rows spmv_sl_min spmv_rw spmv_rw_bounds qa_tile
fs_amx d2h_poll spmv_pair test_build test_math test_dot lmop_mode qf_sparse qf_coop_lds qa_huge qf_split mv_long
fs_long qf_stats route_stats lmop_stats lmop_prune spgemm_dr_sort spat_inc skel_tr fuse_arr spat_stats spgemm_sym
spgemm_sym_stats spgemm_win qf_reuse qf_chain qf_pass qf_grid lmop_wave sg_pattern qa_small lmop_qq_budget
test_qapply test_lmop lmop_small spgemm_flat test_pm test_pm_eager test_fs_select test_fs_expand
test_fs_claim_ext test_fs_vec test_fs_mat test_find_support solve_stats krylov_stats krylov_comm_stats
test_kry_mdot_ranks test_kry_norm_ranks test_kry_spmv_part krylov_n_stats kry_slots kry_family test_kry_spmv_n
test_kry_mdot_n test_kry_update_n kry_tile test_kry_mdot test_kry_update solve_n_stats vc_mrhs_k vc_row_max
vc_mrhs_family test_vc_level_n test_vc_restrict_n vc_fused vc_coop vc_rw vc_tail vc_halo vc_repl
solve_comm_stats test_vc_restrict_map test_vc_halo_xch test_vc_level test_vc_restrict""".split()

# wrapper -> (switch it documents, an argument, the switch's value then, its documented reset argument)
WRAPPERS = {
    "resolve_wave": ("resolve_wave", 1, 1, -1), "seg_split": ("seg_split", 0, 0, -1),
    "dot_split": ("dot_split", 0, 0, -1), "dot_spec_min": ("dot_spec_min", 3, 3, -1),
    "spmv_tab": ("spmv_tab", 1, 1, -1), "spmv_sl_min": ("spmv_sl_min", 0, 0, -1),
    "spmv_rw": ("spmv_rw", 16, 16, -1), "spmv_rw_bounds": ("spmv_rw_bounds", 1420, 1420, -1),
    "qa_tile": ("qa_tile", 32, 32, -1), "fs_amx": ("fs_amx", 0, 0, -1), "d2h_poll": ("d2h_poll", 0, 0, -1),
    "spmv_pair": ("spmv_pair", 0, 0, -1), "lmop_mode": ("lmop_mode", 1, 1, -1),
    "qf_sparse": ("qf_sparse", 2, 2, -1), "qf_coop_lds": ("qf_coop_lds", 100, 100, -1),
    "qa_huge": ("qa_huge", 64, 64, -1), "qf_split": ("qf_split", 0, 0, -1), "mv_long": ("mv_long", 8, 8, -1),
    "fs_long": ("fs_long", 8, 8, -1), "lmop_prune": ("lmop_prune", 0, 0, -1),
    "spgemm_dr_sort": ("spgemm_dr_sort", 0, 0, -1), "spat_inc": ("spat_inc", 0, 0, -1),
    "skel_tr": ("skel_tr", 0, 0, -1), "fuse_arr": ("fuse_arr", 0, 0, -1),
    "spgemm_win": ("spgemm_win", 1024, 1024, -1), "qf_reuse": ("qf_reuse", 0, 0, -1),
    "qf_chain": ("qf_chain", 0, 0, -1), "qf_pass": ("qf_pass", 0, 0, -1), "qf_grid": ("qf_grid", 2, 2, 0),
    "lmop_wave": ("lmop_wave", 0, 0, -1), "sg_pattern": ("sg_pattern", 0, 0, -1),
    "qa_small": ("qa_small", 0, 0, -1), "lmop_qq_budget": ("lmop_qq_budget", 1 << 20, 1 << 20, -1),
    "lmop_small": ("lmop_small", 0, 0, -1),
    "kry_slots": ("kry_slots", 3, 3, -1), "kry_family": ("kry_family", "long", 2, -1),
    "vc_mrhs_k": ("vc_mrhs_k", (4, 2), 6, -1), "vc_row_max": ("vc_row_max", 16, 16, 0),
    "vc_mrhs_family": ("vc_mrhs_family", "short", 1, -1), "vc_fused": ("vc_fused", 0, 0, -1),
    "vc_coop": ("vc_coop", 1, 1, -1), "vc_rw": ("vc_rw", 16, 16, 0), "vc_tail": ("vc_tail", 200, 200, -1),
    "vc_halo": ("vc_halo", 0, 0, -1), "vc_repl": ("vc_repl", 0, 0, -1),
}


def test_public_wrappers_kept(clean_env):
    missing = [f for f in PARENT_API if not callable(getattr(oa, f, None))]
    assert not missing, missing
    assert set(WRAPPERS) <= set(PARENT_API)
    for fn, (name, arg, value, reset) in WRAPPERS.items():
        dflt = oa.knob_get(name)[0]
        getattr(oa, fn)(arg)
        assert oa.knob_get(name) == (value, 2), fn
        getattr(oa, fn)(reset)
        assert oa.knob_get(name) == (dflt, 0), fn
    oa.spgemm_flat(True)                              # no reset value: False is "automatic", set
    assert oa.knob_get("spgemm_flat") == (1, 2)
    oa.spgemm_flat(False)
    assert oa.knob_get("spgemm_flat") == (0, 2)
    oa.knob("spgemm_flat", None)
    oa.qf_grid(-1)                                    # "0 (or -1)"
    assert oa.knob_get("qf_grid")[1] == 0
    oa.vc_mrhs_k(())                                  # no group size: every column alone
    assert oa.knob_get("vc_mrhs_k") == (0, 2)
    oa.vc_mrhs_k(-1)


def test_integration_md_lists_the_tables_variables():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    in_doc = set(re.findall(r"\bAMGD_[A-Z][A-Z0-9_]*\b", doc)) - {"AMGD_TESTS_EXTENDED"}
    in_table = {e["env"] for e in oa.knobs() if e["env"]}
    assert in_doc - NOT_SWITCHES == in_table, sorted((in_doc - NOT_SWITCHES) ^ in_table)
    assert NOT_SWITCHES <= in_doc
    head = open(os.path.join(CSRC, "amgd_knob.h")).read().split("#ifndef")[0]
    assert all(v in head for v in NOT_SWITCHES)


def test_sources_read_the_environment_through_the_table():
    """no getenv of a library variable outside amgd_knob.c and the non-switch sites; no test
    hook left that only forwards an integer to a setter"""
    for path in glob.glob(os.path.join(CSRC, "*")):
        if not path.endswith((".c", ".h", ".hip")) or path.endswith("amgd_knob.c"):
            continue
        src = open(path).read()
        for var in re.findall(r'getenv\(\s*"(AMGD_[A-Z0-9_]+)"', src):
            assert var in NOT_SWITCHES, (os.path.basename(path), var)
        assert not re.search(r"getenv\(\s*[a-z_]", src), path    # nor through a helper's argument
    api = open(os.path.join(CSRC, "amgd_testapi.c")).read()
    forwarders = re.findall(r"^API void (amgd_test_\w+)\((?:u?int(?:32_t|64_t)?|int) \w+\) *\{ *amgd_\w*set\w*\([^;]*\); *\}",
                            api, flags=re.M)
    # kept: a byte count that seven GPU test modules pass through raw ctypes (0: no cap, an override too)
    assert forwarders == ["amgd_test_hbm_cap"], forwarders


def test_table_alone_under_host_sanitizers(tmp_path):
    """amgd_knob.c with tests/knob_check.c, address and undefined-behaviour sanitizers, on the
    host: set, clear and re-read over the whole table, long and malformed values, unknown names"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path / "knob_check")
    # the runtimes linked into the program itself: it runs whatever else the process environment loads
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "knob_check.c"),
                    os.path.join(CSRC, "amgd_knob.c"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == len(oa.knobs())
