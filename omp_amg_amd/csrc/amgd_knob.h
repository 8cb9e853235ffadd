/*
 * amgd_knob.h -- the one table of the library's tuning switches (plain C11, no HIP).
 *
 * A switch's effective value is its override (amgd_knob_set: tests, A/B tools) if one is set,
 * else its environment variable's value, else the default below.  The environment is read on
 * the first amgd_knob() of the process and again at the start of every setup
 * (amgd_drv_stats_begin); a variable that is unset or empty means the default, anything else is
 * strtoll base 10 unless the line names a parse function (amgd_knob.c).  DESIGN.md "Switches".
 *
 * Variables the library reads that are not switches and stay at their sites: AMGD_DUMP (a
 * directory), AMGD_TRACE_MAX_IT and AMGD_TRACE_MAX_S (amgd_setup.c, diagnostics: limits that end the process).
 *
 * X(id, test-side name, environment name or NULL, default, parse function or 0, description)
 */
#ifndef AMGD_KNOB_H
#define AMGD_KNOB_H
#include <stdint.h>

#define AMGD_KNOBS(X)                                                                                        \
  /* runtime (amgd_rt.hip) */                                                                                \
  X(ARENA_GB, "arena_gb", "AMGD_ARENA_GB", -1, 0, "cap on the arena's size in whole GB (-1: free HBM less a margin)") \
  X(HBM_CAP, "hbm_cap", "AMGD_HBM_CAP_GB", 0, amgd_knob_parse_gb, "cap on live device bytes (0: none); the variable is in GB, fractions allowed") \
  X(POISON, "poison", "AMGD_POISON", 0, 0, "1: arrays of doubles start as NaNs (tests)")                   \
  X(D2H_POLL, "d2h_poll", "AMGD_D2H_POLL", 1, 0, "small readbacks polled from host-coherent memory (1) or blocking copies (0)") \
  X(RESOLVE_WAVE, "resolve_wave", "AMGD_RESOLVE", 0, amgd_knob_parse_resolve, "exact sums resolved by one 1024-thread block (0) or one wavefront (1, AMGD_RESOLVE=wave)") \
  X(SEGSTAT, "segstat", "AMGD_SEGSTAT", 0, 0, "1: exact-sum counters printed at exit")                      \
  X(SEG_SPLIT, "seg_split", "AMGD_SEG_SPLIT", 1, 0, "long-row exact sums: split records (0: binade scan; turns off dot_split too)") \
  X(DOT_SPLIT, "dot_split", "AMGD_DOT_SPLIT", 1, 0, "exact dots: split records (0: binade scan)")           \
  X(DOT_SPEC_MIN, "dot_spec_min", "AMGD_DOT_SPEC_MIN", 16, 0, "exact dots: 4096-product chunks from which the chunk speculation runs") \
  X(FAST_DOTS, "fast_dots", "AMGD_FAST_DOTS", 0, 0, "1: plain reductions until amgd_set_exact says otherwise") \
  /* communicator and partitioned primitives (amgd_comm.hip, amgd_part.hip, amgd_psetup.c) */                \
  X(SHARD_MIN, "shard_min", "AMGD_SHARD_MIN", 1000000, amgd_knob_parse_micro, "scale of the sharding work thresholds, in millionths (the variable is a decimal factor)") \
  X(COMM_CHECK, "comm_check", "AMGD_COMM_CHECK", 0, 0, "1: the collective-consistency guard")                \
  X(COMM_SITES, "comm_sites", "AMGD_COMM_SITES", 0, 0, "1: collectives counted per call site")               \
  X(EAGER_SLOT, "eager_slot", "AMGD_EAGER_SLOT", 0, 0, "fixed eager-exchange slot in bytes, at least 8 (0: adaptive)") \
  X(PART_LMOP_GATHER, "part_lmop_gather", "AMGD_PART_LMOP_GATHER", 0, 0, "1: every partitioned interp_lmop on gathered data") \
  /* setup drivers (amgd_drv.c, amgd_setup.c, amgd_psetup.c) */                                              \
  X(VERBOSE, "verbose", "AMGD_VERBOSE", 0, 0, "1: the reference's progress lines on rank 0")                \
  X(PHASES, "phases", "AMGD_PHASES", 0, 0, "1: per-phase times and HBM peaks on stderr")                    \
  X(CS_INC, "cs_inc", "AMGD_CS_INC", 1, 0, "coarsening: incremental sweeps (0: whole sweeps)")             \
  X(CS_MIN_ROWS, "cs_min_rows", "AMGD_CS_MIN_ROWS", 65536, 0, "coarsening: rows from which the sweeps are incremental") \
  X(CS_LIST_NNZ, "cs_list_nnz", "AMGD_CS_LIST_NNZ", 12, 0, "coarsening: mean row length up to which listed rows take one thread each") \
  X(CLOG, "clog", "AMGD_CLOG", 0, 0, "1: a line every tenth coarsening sweep")                              \
  X(SKEL_TR, "skel_tr", "AMGD_SKEL_TR", 1, 0, "skeleton transposes by the transpose map (0: by the sort)") \
  X(FUSE_ARR, "fuse_arr", "AMGD_FUSE_ARR", 1, 0, "W.*(Arhat + Ar) without forming the sum (0: mpm then mxmpoint)") \
  X(SPAT_INC, "spat_inc", "AMGD_SPAT_INC", 1, 0, "constraint pattern grown from the previous iteration's (0: whole product)") \
  X(FS_AMX, "fs_amx", "AMGD_FS_AMX", 1, 0, "find_support selects from the fused first maxima (0: its own pass)") \
  X(FS_INC, "fs_inc", "AMGD_FS_INC", 1, 0, "find_support incremental sweeps: 0 off, 1 from 4096 rows, 2 at every size") \
  X(FSLOG, "fslog", "AMGD_FSLOG", 0, 0, "1: a line per find_support sweep")                                 \
  /* interpolation kernels (amgd_interp.hip, amgd_lmop.hip) */                                               \
  X(QF_SPARSE, "qf_sparse", "AMGD_QF_SPARSE", 1, 0, "huge-support Q factor: 0 dense, 1 sparse first, 2 sparse with a tiny capacity") \
  X(QF_BLOCKED, "qf_blocked", "AMGD_QF_BLOCKED", 1, 0, "33..1024-point Q factors by the blocked kernel (0: k_qfactor_mid)") \
  X(QF_CHAIN, "qf_chain", "AMGD_QF_CHAIN", 1, 0, "blocked Q factor: register rows and read-ahead chains") \
  X(QF_PASS, "qf_pass", "AMGD_QF_PASS", 1, 0, "blocked Q factor, 512 / 1024 tiers: grouped LDS reads in the passes") \
  X(QF_GRID, "qf_grid", NULL, 0, 0, "blocks per launch of the blocked Q-factor tiers (0: the default caps)") \
  X(QF_COOP_LDS, "qf_coop_lds", NULL, 8192, 0, "dense huge-support factor: points up to which s1/s2/qk stay in LDS (at most QF_COOP_MAX of amgd_interp.hip, the same 8192)") \
  X(QF_SPLIT, "qf_split", "AMGD_QF_SPLIT", 1, 0, "huge supports factored per connected component")         \
  X(QF_REUSE, "qf_reuse", "AMGD_QF_REUSE", 1, 0, "unchanged supports copy the previous iteration's factor") \
  X(QA_TILE, "qa_tile", "AMGD_QA_TILE", 16, 0, "Q application, 33..512 points: LDS tile width 16 / 32 (0: row per lane)") \
  X(QA_SMALL, "qa_small", "AMGD_QA_SMALL", 1, 0, "Q application: supports of <= 32 points on the lane-group kernels") \
  X(QA_HUGE, "qa_huge", NULL, 8192, 0, "Q application: points above which the grid-wide kernels run")      \
  X(LMOP_WAVE, "lmop_wave", "AMGD_LMOP_WAVE", -1, 0, "interp_lmop general walk per wavefront from this support size (0: never; -1: from 64, the pruned walk never)") \
  X(LMOP_PRUNE, "lmop_prune", "AMGD_LMOP_PRUNE", 4096, 0, "general walk: support size from which split supports are pruned (0: never)") \
  X(LMOP_SMALL, "lmop_small", "AMGD_LMOP_SMALL", 1, 0, "row pull: S rows of <= 32 entries one thread each") \
  X(LMOP_QQ_BUDGET, "lmop_qq_budget", "AMGD_QQ_BUDGET_MB", 17179869184, amgd_knob_parse_mb, "row pull: bytes of QQ^t formed at a time, at least 1 MB; the variable is in whole MB") \
  X(LMOP_MODE, "lmop_mode", "AMGD_LMOP", 0, amgd_knob_parse_lmop, "interp_lmop: 0 row pull where order-exact, 1 general walk (AMGD_LMOP=general)") \
  X(FS_LONG, "fs_long", "AMGD_FS_LONG", -1, 0, "find_support: row length past which the grid-wide kernels run (0: never; -1: max(4096, 16 x mean))") \
  X(SGLOG, "sglog", "AMGD_SGLOG", 0, 0, "1: a line per SpGEMM, Q factor, support split and pruned walk")    \
  /* SpMV and SpGEMM (amgd_sparse.hip) */                                                                    \
  X(SL_MIN_ROWS, "sl_min_rows", "AMGD_SL_MIN_ROWS", 4096, 0, "long-row SpMV: rows from which the lane kernel runs") \
  X(SL_LIST_MIN_ROWS, "sl_list_min_rows", "AMGD_SL_LIST_MIN_ROWS", 4096, 0, "the same for listed-row products") \
  X(SPMV_SL_MIN, "spmv_sl_min", NULL, -1, 0, "both of the above at once (-1: each its own)")               \
  X(SPMV_TAB, "spmv_tab", "AMGD_MV_TAB", 0, 0, "1: gather tables for pinned long-row matrices")             \
  X(SPMV_PAIR, "spmv_pair", "AMGD_MV_PAIR", 1, 0, "products with x through k_spmv_pair (0: k_spmv_pipe)")   \
  X(SPMV_RW, "spmv_rw", "AMGD_SL_RW", 0, 0, "lane SpMV: rows per wavefront 4 / 16 / 64 (else by row count)") \
  X(SPMV_RW_BOUNDS, "spmv_rw_bounds", NULL, 1622, 0, "lane SpMV: log2 row counts of the 16 / 64-row shapes as lo * 100 + hi") \
  X(MV_LONG, "mv_long", "AMGD_MV_LONG", -1, 0, "listed products: row length past which the exact block kernel runs (0: never; -1: max(4096, 16 x mean))") \
  X(MVLOG, "mvlog", "AMGD_MVLOG", 0, 0, "1: a line per whole-matrix SpMV")                                  \
  X(MVSTAT, "mvstat", "AMGD_MVSTAT", 0, 0, "1: x locality of pinned long-row matrices (analysis)")          \
  X(DR_SORT, "spgemm_dr_sort", "AMGD_DR_SORT", 1, 0, "SpGEMM rows past the hash bins by sorting (0: the dense-slab kernel)") \
  X(SG_FLAT, "spgemm_flat", "AMGD_SG_FLAT", 0, 0, "1: flat-enumeration SpGEMM kernels only")                \
  X(SG_WIN, "spgemm_win", "AMGD_SG_WIN", 2048, 0, "SpGEMM wide rows: window 1024..16384 (0: hash kernels only); an override > 0 windows every wide row") \
  X(SG_WIN_P0, "spgemm_win_p0", "AMGD_SG_WIN_P0", 48, 0, "products per window from which a wide row is windowed") \
  X(SG_TINY, "spgemm_tiny", "AMGD_SG_TINY", 1, 0, "SpGEMM rows of few products one thread each")            \
  X(SG_PATTERN, "sg_pattern", NULL, 1, 0, "constraint pattern by the pattern-only product (0: full product)") \
  /* solve (amgd_vcycle.c, amgd_solve.hip, amgd_krylov.c) */                                                 \
  X(VC_FUSED, "vc_fused", "AMGD_VC_FUSED", 1, 0, "V-cycle by the fused kernels (0: composed)")              \
  X(VC_COOP, "vc_coop", "AMGD_VC_COOP", 0, 0, "1: long-row shapes by the cooperative kernels (0: composed)")   \
  X(VC_TAIL, "vc_tail", "AMGD_VC_TAIL", 1, 0, "one-workgroup coarse tail; the variable is on / off, an override a row count (at most 1024) that is the only limit") \
  X(VC_TAIL_WORK, "vc_tail_work", "AMGD_VC_TAIL_WORK", 16384, 0, "work limit of the coarse tail")        \
  X(VC_HALO, "vc_halo", "AMGD_VC_HALO", 1, 0, "partitioned V-cycle: halo lists (0: allgatherv)")            \
  X(VC_REPL, "vc_repl", "AMGD_VC_REPL_ROWS", 32768, 0, "partitioned V-cycle: slice size up to which levels are replicated") \
  X(VC_ROW_MAX, "vc_row_max", NULL, 4096, 0, "solve plans: row length past which a row is an outlier (0: VC_ROW_MAX of amgd_vcycle.c, the same 4096)") \
  X(VC_RW, "vc_rw", NULL, 0, 0, "cooperative V-cycle kernels: rows per wavefront 4 / 16 / 64 (else by row count)") \
  X(VC_MRHS_K, "vc_mrhs_k", "AMGD_VC_MRHS_K", 14, amgd_knob_parse_ksizes, "multi-RHS group sizes as a mask of 2 | 4 | 8 (AMGD_VC_MRHS_K=8,4,2; 0: none)") \
  X(VC_MRHS_FAMILY, "vc_mrhs_family", "AMGD_VC_MRHS_FAMILY", 0, 0, "multi-RHS kernel family: 0 by row shape, 1 short-row, 2 long-row") \
  X(KRY_SLOTS, "kry_slots", "AMGD_KRY_SLOTS", 8, 0, "slots of the lock-step Krylov solver (1..8; less than 1: KRY_SLOTS_DEFAULT of amgd_krylov.c, the same 8)")          \
  X(KRY_FAMILY, "kry_family", "AMGD_KRY_MRHS_FAMILY", 0, 0, "its product's kernel family: 0 by mean row length, 1 short-row, 2 long-row")

#define AMGD_KNOB_ID(id, name, env, dflt, parse, doc) AMGD_K_##id,
enum { AMGD_KNOBS(AMGD_KNOB_ID) AMGD_K_N };
#undef AMGD_KNOB_ID

#ifdef __cplusplus
extern "C" {
#endif
extern int64_t amgd_knob_val[AMGD_K_N];   /* effective values */
extern int amgd_knob_ready;
void amgd_knobs_read_env(void);           /* (re)read every entry's variable */
int amgd_knob_source(int id);             /* 0 default, 1 environment, 2 override */
void amgd_knob_set(int id, int64_t v);
void amgd_knob_clear(int id);
/* the table, for the test hooks: id of a test-side name (-1: none) and entry by index */
int amgd_knob_find(const char *name);
int amgd_knob_info(int id, const char **name, const char **env, int64_t *dflt);
static inline int64_t amgd_knob(int id) {
  if (!amgd_knob_ready) amgd_knobs_read_env();
  return amgd_knob_val[id];
}
#ifdef __cplusplus
}
#endif
#endif
