/*
 * amgd.h -- the thin internal C ABI between the host setup driver (amgd_setup.c,
 * plain C) and the hand-written HIP kernels (amgd_*.hip).  No HIP or torch type
 * appears here: device memory is passed as plain pointers, matrices as `dcsr`.
 *
 * Device CSR layout in HBM (DESIGN.md "Data layout"):
 *   ro  : u64[rn+1]  row offsets (64-bit: coarse operators exceed 2^32 nnz at scale)
 *   col : u32[nnz]   column indices, ascending within a row (reference invariant)
 *   a   : f64[nnz]   values
 * Masks (C/F sets, strength filters) are u8 {0,1} arrays; the reference keeps
 * them as doubles (amg_setup.c:175-180) but every use is a !=0 test or a
 * multiply by 0/1 of a non-negative value, which the u8 form reproduces exactly.
 */
#ifndef AMGD_H
#define AMGD_H

#include <stddef.h>
#include <stdint.h>

#include "amgd_knob.h"      /* the tuning switches: amgd_knob(AMGD_K_...) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t rn, cn;
  uint64_t nnz;
  uint64_t *ro;
  uint32_t *col;
  double *a;
} dcsr;

/* ---------------- runtime (amgd_rt.hip) ---------------- */
int amgd_rt_init(int device);            /* idempotent; 0 on success */
const char *amgd_last_error(void);
void amgd_set_error(const char *msg);
void *amgd_alloc(size_t bytes);          /* arena; out of HBM: unwinds to amgd_try, else aborts */
void *amgd_alloc_f64(size_t bytes);      /* the same, for arrays of doubles (AMGD_POISON=1: NaN-filled) */
/* run fn(arg); if an allocation runs out of HBM inside it, every block allocated since
   the call is released and -2 returned (amgd_last_error() has the text) */
int amgd_try(int (*fn)(void *), void *arg);
void amgd_spmv_split_clear(void);        /* drop every cached SpMV shard split */
/* reset the per-call module state a setup sets and clears around its kernels (SpGEMM
   pattern mode / timer slot, Q-factor reuse pointers, component-split depth): called at the
   start of every setup and after an unwound one */
void amgd_reset_call_state(void);
void amgd_sparse_reset_state(void);
void amgd_interp_reset_state(void);
void amgd_free(void *p);
uint32_t amgd_max_row_len(const dcsr *M);   /* longest row of a pinned matrix, else UINT32_MAX */
void amgd_rowmax_pin(const dcsr *M);           /* pattern fixed until unpinned / freed */
void amgd_rowmax_unpin(const dcsr *M);
void amgd_spmv_split_forget(const void *ro);   /* drop cached SpMV shard splits of a freed buffer */
/* partitioned-setup diagnostics (tests): interp_lmop calls on gathered data / with a dirty
   prefix; eager exchanges / those that took the second round; forced rare paths */
void amgd_part_stats(uint64_t *out2);
void amgd_spmv_tab_stats(uint64_t *out3);       /* gather-table builds, tiles, direct tiles */
void pm_eager_stats(uint64_t *calls, uint64_t *second);
void amgd_rt_shutdown(void);             /* free everything; pointers become invalid */
void amgd_pool_release(void);            /* return every cached block to the driver */
size_t amgd_pool_bytes_in_use(void);
size_t amgd_pool_peak_bytes(void);
void amgd_pool_peak_reset(void);
size_t amgd_pool_ipeak_take(void);        /* peak since the last call, then reset */          /* peak := bytes in use now (start of a setup) */
void amgd_pool_stats(uint64_t *nmalloc, double *gbytes, double *ms, uint64_t *nrelease);
void amgd_h2d(void *d, const void *h, size_t n);
void amgd_d2h(void *h, const void *d, size_t n);
void amgd_d2d(void *d, const void *s, size_t n);
void amgd_memset(void *d, int v, size_t n);
void amgd_sync(void);
double amgd_wtime(void);
void *amgd_stream(void);                 /* hipStream_t of the library */
void amgd_set_stream(void *stream);
/* event timers on the library stream, for kernel-level throughput */
void amgd_timer_start(int slot);
void amgd_timer_stop(int slot);
void amgd_timer_start2(int slot, int slot2);   /* two slots timing the same interval */
void amgd_timer_stop2(int slot, int slot2);
double amgd_timer_ms(int slot);          /* accumulated, syncs */
void amgd_timer_reset(void);
void amgd_timers_enable(int on);         /* 0: start / stop record nothing (inside a solve) */
/* the solve side's own event timers, which amgd_timer_reset and amgd_timers_enable do not touch:
   the single-vector cycles (amgd_solve_stats), the multi-RHS calls (amgd_solve_n_stats), the
   Krylov solves (amgd_krylov_stats), the multi-RHS Krylov calls (amgd_krylov_n_stats).  _end
   reads the pending event pairs back once 256 wait on the timer -- for a timer whose interval
   encloses cycles, on it and the cycles' timer together, and it reads both; _ms reads them and
   returns the milliseconds so far (syncs); _zero also clears the sum */
enum { AMGD_XT_VC = 0, AMGD_XT_VCN, AMGD_XT_KRY, AMGD_XT_KRYN, AMGD_XT_N };
void amgd_xtimer_begin(int id);
void amgd_xtimer_end(int id);
double amgd_xtimer_ms(int id);
void amgd_xtimer_zero(int id);
uint64_t amgd_timer_pending(void);       /* event pairs waiting to be read, every timer (tests) */
void amgd_spgemm_set_timer(int slot);     /* SpGEMM numeric kernels timed on slot (-1: off) */

dcsr *dcsr_new(uint32_t rn, uint32_t cn, uint64_t nnz);
void dcsr_free(dcsr **A);
dcsr *dcsr_copy(const dcsr *A);
dcsr *dcsr_empty_like_pattern(const dcsr *A);   /* same ro/col, fresh a */

/* kernel-route counters (which default paths a setup took; read by the parity tests
   at sizes where the default routing engages) */
enum { AMGD_R_SPMV_PIPE, AMGD_R_MV_LONG, AMGD_R_SG_TINY, AMGD_R_SG_KSEQ, AMGD_R_SG_WWIN,
       AMGD_R_SG_WWIN_SYM, AMGD_R_SG_LONG, AMGD_R_CS_INC, AMGD_R_FS_INC, AMGD_R_SG_ROW,
       AMGD_R_MV_RW4, AMGD_R_QF_REUSE, AMGD_R_LMOP_WAVE, AMGD_R_MV_RW16, AMGD_R_MV_RW64,
       AMGD_R_QF_T512, AMGD_R_QF_T1024, AMGD_R_MV_PAIR, AMGD_R_FS_AMX, AMGD_R_MV_TAB, AMGD_R_SG_SYMREUSE, AMGD_R_SPAT_INC, AMGD_R_SG_DRSORT, AMGD_R_SKEL_TR,
       AMGD_R_FS_SWEEP,     /* every pass of find_support's loop (one-GPU driver) */
       /* V-cycle products by form: thread per row, cooperative long-row, composed from the
          setup's kernels; cycles whose deepest levels ran in the one-workgroup tail */
       AMGD_R_VC_THR, AMGD_R_VC_WAVE, AMGD_R_VC_COMP, AMGD_R_VC_TAIL,
       /* partitioned V-cycle (amgd_vcycle.c): halo exchanges, allgather exchanges, cycles
          that ran replicated coarse levels */
       AMGD_R_VC_HALO, AMGD_R_VC_ALLG, AMGD_R_VC_REPL,
       /* Q application launches by kernel: <= 16 / 17..32 points in lane groups, 33..512
          (whichever tile), the 256-thread block kernel; QA_HUGE counts supports */
       AMGD_R_QA_S16, AMGD_R_QA_S32, AMGD_R_QA_MID, AMGD_R_QA_BLK, AMGD_R_QA_HUGE,
       /* interp_lmop row pull launches: thread / wavefront / 256-thread block per S row, the
          tiled QQ^t kernel; LMOP_CHUNKS counts the QQ^t chunks of every call */
       AMGD_R_LMOP_PULL_THR, AMGD_R_LMOP_PULL_WAVE, AMGD_R_LMOP_PULL_BLK, AMGD_R_LMOP_QQ_TILE,
       AMGD_R_LMOP_CHUNKS,
       /* multi-RHS V-cycle (amgd_solve_device_n): products by kernel family (short-row /
          long-row K-column kernels), columns sent through the single-vector cycle (a leftover),
          columns of one level's restriction or up-sweep run through the single-vector code
          (a matrix with an outlier row) */
       AMGD_R_VC_MR_THR, AMGD_R_VC_MR_WAVE, AMGD_R_VC_MR_SINGLE, AMGD_R_VC_MR_COMP,
       /* flexible GMRES (amgd_krylov.c): inner iterations, fused multi-dot launches, ordered dots */
       AMGD_R_KRY_IT, AMGD_R_KRY_MDOT, AMGD_R_KRY_ODOT,
       /* flexible GMRES on several right-hand sides (amgd_krylov_device_n): lock-step steps,
          steps whose active columns stood at two or more different j, K-column product
          launches, columns sent through the single-vector cycle or product as a group's
          leftover, per-column products of an outlier-row matrix */
       AMGD_R_KRY_N_STEP, AMGD_R_KRY_N_MIXED, AMGD_R_KRY_N_PROD, AMGD_R_KRY_N_SINGLE, AMGD_R_KRY_N_COMP,
       /* flexible GMRES on a row-partitioned hierarchy: exchanges before a level-0 product,
          rank-order combines of the ranks' partial sums */
       AMGD_R_KRY_P_XCH, AMGD_R_KRY_P_COMB,
       AMGD_R_N };
extern uint64_t amgd_route_ctr[AMGD_R_N];
#define amgd_route_hit(r) (amgd_route_ctr[(r)]++)

/* scans: counts[0..n-1] -> exclusive prefix in counts[0..n], returns total */
uint64_t amgd_scan_u64(uint64_t *counts, uint64_t n);
uint32_t amgd_scan_u32(uint32_t *counts, uint64_t n);
/* compaction map for a u8 mask: map[i] = rank of i among set entries (or ~0) */
uint32_t amgd_mask_rank(const uint8_t *mask, uint32_t n, uint32_t *map);

/* AMGD_PHASES=1 phase profile (amgd_setup.c): time of the phase just ended on a level */
enum { PH_COARSEN, PH_SMOOTH, PH_IPRE, PH_QF, PH_W0, PH_SPAT, PH_LMOP, PH_PCG, PH_W, PH_AFW, PH_R,
       PH_FS, PH_FS_MV, PH_FS_MAX, PH_FS_SEL, PH_EXP, PH_EXP_R0, PH_FINAL, PH_RAP, PH_N };
void amgd_ph_mark(int lvl, int id);      /* -1: restart the clock */
void amgd_ph_report(uint32_t nlevels);

/* ---------------- row sharding over GPUs (amgd_comm.hip) ---------------- */
int amgd_nshards(void);                          /* 1: sharding off */
int amgd_comm_procs(void);                       /* processes of the communicator (sim: 1) */
void amgd_my_shards(int *first, int *last);      /* shard ranges this process computes */
int amgd_shard_worth(uint64_t work, uint64_t min_work);
/* contiguous ranges of equal work: split_h[0..N] from an exclusive prefix of n+1 entries */
void amgd_shard_split(const uint64_t *prefix, uint32_t n, uint32_t *split_h);
/* Collectives.  Each records its call site (file:line of the outermost caller) for the
   collective-consistency guard (AMGD_COMM_CHECK=1 / amgd_comm_set_check): before every
   collective the ranks exchange (sequence number, kind, call site, offsets signature,
   send lengths) in a fixed-size record and abort naming both ranks' sites on any
   mismatch -- a rank-local skip or a size disagreement cannot go unnoticed (RCCL would
   hang or corrupt).  The same record carries an out-of-HBM on one rank to all of them,
   so every rank unwinds its setup together (amgd_comm_fail_agree). */
void amgd_comm_site(const char *file, int line);
int amgd_comm_fail_agree(void);    /* 1: every rank was told of this rank's failure */
void amgd_comm_site_report(void);  /* AMGD_COMM_SITES=1: collectives per call site (stderr) */
/* range s of buffer b = bytes [off[b*(N+1)+s], off[b*(N+1)+s+1]), completed on every rank */
void amgd_allgatherv_(int nbuf, void *const *bufs, const uint64_t *off);
#define amgd_allgatherv(...) (amgd_comm_site(__FILE__, __LINE__), amgd_allgatherv_(__VA_ARGS__))
void amgd_allgather_u64_(uint64_t *vals_h);      /* vals_h[s] of the own shards -> all */
#define amgd_allgather_u64(...) (amgd_comm_site(__FILE__, __LINE__), amgd_allgather_u64_(__VA_ARGS__))
void amgd_gather_u64_at(const uint64_t *a, const uint32_t *idx_h, int n, uint64_t *out_h);

/* partitioned mode (amgd_psetup.c): ranks own row blocks; amgd_nshards() is 1 there */
int amgd_comm_partitioned(void);
void amgd_comm_suspend_partition(int on);
int amgd_comm_part_default(void);
int amgd_comm_part_get(void);          /* raw flag: -1 unset, 0 off, 1 on */
void amgd_comm_part_set(int v);
/* calls, bytes of: data allgatherv, alltoallv, small u64 allgathers (since the last reset) */
void amgd_comm_stats_kind(uint64_t *out6);
int amgd_pcomm_rank(void);
int amgd_pcomm_size(void);
void amgd_pcomm_allgather_u64_(uint64_t *vals_h, int m);  /* vals_h[N*m]: own m -> all */
#define amgd_pcomm_allgather_u64(...) (amgd_comm_site(__FILE__, __LINE__), amgd_pcomm_allgather_u64_(__VA_ARGS__))
/* rank sends send[soff[p]..soff[p+1]) to p, receives p's into recv[roff[p]..roff[p+1]) (bytes) */
void amgd_pcomm_alltoallv_(const void *send, const uint64_t *soff, void *recv, const uint64_t *roff);
#define amgd_pcomm_alltoallv(...) (amgd_comm_site(__FILE__, __LINE__), amgd_pcomm_alltoallv_(__VA_ARGS__))
/* nb such exchanges (buffers b = 0..nb-1) in one collective */
void amgd_pcomm_alltoallv_n_(int nb, const void *const *send, const uint64_t *const *soff, void *const *recv,
                             const uint64_t *const *roff);
#define amgd_pcomm_alltoallv_n(...) (amgd_comm_site(__FILE__, __LINE__), amgd_pcomm_alltoallv_n_(__VA_ARGS__))

/* ---------------- reductions (return host values, sync) ---------------- */
void amgd_set_exact(int on);     /* 1: reference-order (sequential) dots -- default; 0: tree */
int amgd_get_exact(void);
double amgd_dot(const double *a, const double *b, uint64_t n);
double amgd_norm2(const double *a, uint64_t n);
double amgd_max_first(const double *a, uint64_t n, uint64_t *idx);  /* first argmax */
double amgd_max_first2(const double *a, const double *b, uint64_t n, uint64_t *idx, double *maxb);
uint64_t amgd_count_gt(const double *a, uint64_t n, double thr, double *maxv);
double amgd_fro_minus_eye(const dcsr *A);                          /* ||A - I||_F^2 */

/* ---------------- sparse (amgd_sparse.hip) ---------------- */
dcsr *amgd_build_csr(uint64_t nz, const uint32_t *Ai, const uint32_t *Aj, const double *Av);
dcsr *amgd_coo2csr(uint64_t nz, const uint32_t *I, const uint32_t *J, const double *V,
                   uint32_t rn, uint32_t cn, int drop_zero);
dcsr *amgd_sub_mat(const dcsr *A, const uint8_t *vr, const uint8_t *vc);
dcsr *amgd_transpose(const dcsr *A, uint64_t **perm_out);
dcsr *amgd_drop_zeros(const dcsr *A);                      /* exactly-zero entries removed */
dcsr *amgd_rows_masked(const dcsr *A, const uint8_t *mask);  /* rows with mask==0 emptied */
dcsr *amgd_cols_masked(const dcsr *A, const uint8_t *mask);  /* entries with mask[col]==0 dropped */
uint64_t *amgd_perm_inverse(const uint64_t *p, uint64_t n);  /* q[p[t]] = t */
/* values through the map perm of T = amgd_transpose(A, &perm), no sort: a new matrix on
   pattern's ro / col (copied) with a[perm[t]] = vt[t] -- the transpose of the matrix (T's
   pattern, vt) when pattern is A's and amgd_rows_strict(A); and T->a[t] = a[perm[t]], the
   transpose of the matrix (A's pattern, a), written into T */
dcsr *amgd_untranspose_by_perm(const dcsr *pattern, const uint64_t *perm, const double *vt);
void amgd_transpose_by_perm(dcsr *T, const uint64_t *perm, const double *a);
int amgd_rows_strict(const dcsr *A);      /* 1: every row's columns strictly increasing (syncs) */
dcsr *amgd_spgemm(const dcsr *A, const dcsr *B);           /* A*B, reference semantics */
/* pattern of A*B, values unspecified nonzeros (operands with all values > 0) */
dcsr *amgd_spgemm_pattern(const dcsr *A, const dcsr *B);
/* the next one-GPU product: 1 keeps its symbolic phase, 2 takes the kept one when both
   operand patterns match (else runs in full); drop frees a kept state */
void amgd_spgemm_sym_next(int mode);
void amgd_spgemm_sym_drop(void);
void amgd_spgemm_sym_stats(uint64_t *kept, uint64_t *reused);
/* the constraint operator's pattern grown from the previous iteration's (amgd_setup.c) */
void amgd_spat_stats(uint64_t *out3);     /* incremental, whole, same pattern */
void amgd_spat_forget(void);
dcsr *amgd_mpm(double alpha, const dcsr *A, double beta, const dcsr *B);
dcsr *amgd_mxmpoint(const dcsr *A, const dcsr *B);
/* amgd_mxmpoint(A, amgd_mpm(1., B1, 1., B2)), the sum never formed */
dcsr *amgd_mxmpoint_sum(const dcsr *A, const dcsr *B1, const dcsr *B2);
/* z =(y ? alpha*y + beta*t : beta*t) [* f] with t = M x summed in column order */
void amgd_spmv(const dcsr *M, const double *x, double *z, double alpha, const double *y,
               double beta, const uint8_t *f);
/* z[list[r]] = row list[r] of M times x (x == NULL: row sums), left to right */
void amgd_spmv_rows(const dcsr *M, const uint32_t *list, uint32_t n, const double *x, double *z);
/* z = M^T x, per column in ascending row order; Mt = transpose(M) */
void amgd_spmvt(const dcsr *Mt, const double *x, double *z);
void amgd_colsum(const dcsr *Mt, double *z);   /* sum(M,1) via Mt */
void amgd_diag(const dcsr *A, double *D);
enum { AMGD_DPLUS = 0, AMGD_DMINUS = 1, AMGD_DMULT = 2, AMGD_MULTD = 3,
       AMGD_SCALE2 = 4, AMGD_SCALE_ABS = 5, AMGD_SCALE2_ABS = 6, AMGD_SCALE_ABS_T = 7 };
void amgd_diag_op(dcsr *A, const double *D, int op);
/* fused: SCALE2 a=(a*Dl[i])*Dr[col]; SCALE_ABS a=|a*Dl[i]|*Dr[col]; SCALE2_ABS a=|(a*Dl[i])*Dr[col]|;
   SCALE_ABS_T a=|a*Dl[col]|*Dr[i] (SCALE_ABS of the transpose, entry by entry) */
void amgd_diag_op2(dcsr *A, const double *Dl, const double *Dr, int op);
void amgd_vals_abs(dcsr *A);
void amgd_vals_sqr(dcsr *A);
void amgd_vals_scale(dcsr *A, double s);
void amgd_rowsum_sq_inv(const dcsr *A, double *s);     /* s_i = 1/sum_j a_ij^2 (row order) */
uint64_t amgd_to_host_cols(const dcsr *A, unsigned long *h_ro, unsigned long *h_col, double *h_a);

/* ---------------- vectors (amgd_vec.hip) ---------------- */
enum {
  AMGD_V_FILL, AMGD_V_INV, AMGD_V_SQRT, AMGD_V_MUL, AMGD_V_ADD, AMGD_V_SUB, AMGD_V_DIV
};
void amgd_vfill(double *a, uint64_t n, double v);
void amgd_vop(double *c, const double *a, const double *b, uint64_t n, int op); /* c = a op b */
void amgd_vunary(double *a, uint64_t n, int op);                                /* a = op(a) */
void amgd_vscale(double *a, uint64_t n, double s);                              /* a = a*s */
void amgd_u8_to_f64(const uint8_t *m, double *d, uint64_t n);
void amgd_compact_ids(const unsigned long *id, const uint8_t *vc, uint32_t n,
                      unsigned long *idc, unsigned long *idf);
void amgd_lanczos_step(const double *r, double rbeta_inv, double *qk, double *qkm1, uint64_t n);
void amgd_lanczos_resid(double *r, const double *Aqk, const double *qk, double alpha,
                        double *qkm1, double beta, uint64_t n);
/* pcg pieces */
void amgd_pcg_p(double *p, const double *z, double beta, uint64_t n);
void amgd_pcg_xrz(double *x, double *r, double *z, const double *p, const double *w,
                  const double *M, double alpha, uint64_t n);
void amgd_vmul_dot_prep(double *z, const double *M, const double *r, uint64_t n);
double amgd_dot3(const double *M, const double *b, uint64_t n);  /* sum (M.*b).*b */

/* ---------------- coarsening (amgd_coarsen.hip) ---------------- */
void amgd_coarsen_w(const double *w1, const double *w2, double *w, uint32_t n);
void amgd_coarsen_mask1(const double *w, double ctol2, const double *g, uint8_t *mask,
                        double *x, uint32_t n);
void amgd_mat_max(const dcsr *S, const dcsr *St, const uint8_t *f, const double *x, double tol,
                  double *amax_tmp, double *y);
void amgd_mat_amax(const dcsr *S, const uint8_t *f, double tol, double *amax);
void amgd_mat_max_gather(const dcsr *St, const uint8_t *f, const double *x, const double *amax,
                         double *y);
void amgd_coarsen_mask2(double *g, const double *m, uint8_t *mask, double *x, uint32_t n);
void amgd_coarsen_mask3(const double *m, uint8_t *mask, uint8_t *vc, uint8_t *vf, double *vfd,
                        uint32_t n, uint32_t *anyvc);
/* incremental sweeps (amgd_coarsen.hip): a stage of radius R runs on the rows
   within R hops of the last sweep's new C points -- the prefix cum[R] of the BFS
   list (list mode) or the rows i with fs[i] - fb <= R (filter mode); rows = NULL
   runs the full kernels */
typedef struct {
  const uint32_t *list;   /* BFS rows in hop order (list mode) or NULL */
  uint32_t cum[8];        /* rows within r hops */
  const uint32_t *fs;     /* row stamps (filter mode) */
  uint32_t fb;            /* 8 * sweep */
} amgd_csrows;
int amgd_cs_grow(const dcsr *S, const dcsr *St, uint32_t *front, uint32_t *cnt_d,
                 uint32_t *stamp, uint32_t base8, uint32_t limit, uint32_t *cum);
/* partitioned mode: one BFS hop of amgd_cs_grow, and the claim of another rank's hop rows */
void amgd_cs_hop1(const dcsr *S, const dcsr *St, uint32_t *front, uint32_t *cnt_d, int r, uint32_t *stamp,
                  uint32_t base8, uint32_t limit);
void amgd_cs_claim_ext(const uint32_t *ids, uint64_t n, uint32_t *stamp, uint32_t base8, int r,
                       uint32_t *front, uint32_t hi0, uint32_t *cntr);
void amgd_spmv_filt(const dcsr *M, const double *x, double *z, const uint8_t *f,
                    const uint32_t *fs, uint32_t fb, uint32_t fr);
void amgd_mat_amax_filt(const dcsr *S, const uint8_t *f, double tol, double *amax,
                        const uint32_t *fs, uint32_t fb, uint32_t fr);
void amgd_mat_max_gather_filt(const dcsr *St, const uint8_t *f, const double *x,
                              const double *amax, double *y, const uint32_t *fs, uint32_t fb,
                              uint32_t fr);
void amgd_cs_spmv(const dcsr *S, const double *x, double *z, const uint8_t *f,
                  const amgd_csrows *rows, uint32_t R);
void amgd_cs_w_mask1(uint32_t n, const double *w1, const double *w2, double *w, double ctol2,
                     const double *g, uint8_t *ma, double *x1, const amgd_csrows *rows,
                     uint32_t R);
void amgd_cs_amax(const dcsr *S, const uint8_t *f, double tol, double *amax,
                  const amgd_csrows *rows, uint32_t R);
void amgd_cs_gather(const dcsr *St, const uint8_t *f, const double *x, const double *amax,
                    double *y, const amgd_csrows *rows, uint32_t R);
void amgd_cs_mask2(uint32_t n, const double *g, const double *m1, const uint8_t *ma, uint8_t *mb,
                   double *x2, const amgd_csrows *rows, uint32_t R);
void amgd_cs_mask3(uint32_t n, const double *m2, const uint8_t *mb, uint8_t *vc, uint8_t *vf,
                   double *vfd, uint32_t *anyvc, uint32_t *d0, uint32_t *d0cnt, uint32_t *stamp,
                   uint32_t next_base8, const amgd_csrows *rows, uint32_t R);

/* ---------------- interpolation (amgd_interp.hip) ---------------- */
dcsr *amgd_min_skel(const dcsr *R);
/* Q factors of A restricted to each row-support of Wt (packed upper triangles) */
double *amgd_qfactor(const dcsr *Wt, const dcsr *A, uint64_t **qoff_out, uint64_t *qtotal);
/* the same, copying the factor of every support identical to the previous call's (Wp, Qp,
   qpoff: that call's Wt, factors and offsets; NULL: factor everything) */
double *amgd_qfactor_reuse(const dcsr *Wt, const dcsr *A, uint64_t **qoff_out, uint64_t *qtotal,
                           const dcsr *Wp, const double *Qp, const uint64_t *qpoff);
void amgd_qfactor_reuse_stats(uint64_t *reused, uint64_t *factored);
void amgd_qapply(const dcsr *Wt, const double *Q, const uint64_t *qoff, const dcsr *Bt,
                 const double *u, const double *lambda, double *out);
/* S := interp_lmop contributions (S pattern = W_skel*W_skel'); kpos from amgd_lmop_kpos */
int amgd_lmop(dcsr *S, const dcsr *Wskel, const uint32_t *kpos, const dcsr *Wt, const double *Q,
              const uint64_t *qoff, const double *u);
uint32_t *amgd_lmop_kpos(const dcsr *Wt, const uint64_t *perm);
void amgd_lmop_stats(uint64_t *out);   /* fast, general, dirty-prefix calls, misses, pruned supports */
void amgd_lmop_stats_reset(void);
void amgd_lmop_spill_detect(int on);   /* partitioned mode: flag walks past the view's last row */
int amgd_lmop_spilled(void);
/* partitioned mode: [0, d) already added to S (the dirty prefix walked on the whole S
   pattern); amgd_lmop then adds [d, nc) only.  0: off */
void amgd_lmop_set_prefix(uint32_t d);
/* amgd_lmop_general keeps the values of S positions [lo, hi) only, in a (NULL: off) */
void amgd_lmop_set_window(double *a, uint64_t lo, uint64_t hi);
/* the exact (sp_add-walk) contributions of the coarse points [cb, ce) added to S */
void amgd_lmop_general(dcsr *S, const dcsr *Wt, const double *Q, const uint64_t *qoff, const double *u,
                       uint32_t cb, uint32_t ce);
void amgd_lmop_classify_view(const dcsr *Wt, uint32_t *dend, uint32_t *cmin);
uint64_t amgd_lmop_qq_bytes(void);    /* QQ^t bytes of the last amgd_lmop call */
int amgd_lmop_missed(void);            /* a clean contribution missed (prefix mode); clears */
void amgd_qfactor_stats(unsigned long *st); /* [sparse, dense fallback, split] since the last call */
/* one find_support sweep: select/remove, then re-sum rs (rows) and sumR (columns) that lost
   an entry */
uint32_t amgd_fs_select(const dcsr *Rl, const dcsr *Rt, const uint64_t *perm, double *rs,
                        const double *w, double *sumR, double thr,
                        uint32_t *sel_i, uint32_t *sel_j, uint32_t *nremoved);
/* the same over rows c0.. of R' (w, sumR at c0; sel_j global); perm NULL: R untouched;
   resum 0: rs / sumR not re-summed (partitioned mode) */
void amgd_list_rowsum(const dcsr *M, const uint32_t *list, uint32_t n, double *out, int long_rows);
uint32_t amgd_fs_select_ex(const dcsr *Rl, const dcsr *Rt, const uint64_t *perm, double *rs,
                           const double *w, double *sumR, double thr, uint32_t *sel_i,
                           uint32_t *sel_j, uint32_t *nremoved, uint32_t c0, int resum);
/* incremental sweeps: distinct columns of the listed rows of M (stamp/tag dedupe);
   returns the count, > cap when the list overflowed */
int amgd_spmv_amax(const dcsr *M, const double *x, double *z, uint64_t *amx);
uint32_t amgd_fs_select_amx(const dcsr *Rl, const dcsr *Rt, const uint64_t *perm, double *rs,
                            const double *w, double *sumR, double thr, const uint64_t *amx,
                            uint32_t *sel_i, uint32_t *sel_j, uint32_t *nremoved);
uint32_t amgd_fs_expand(const dcsr *M, const uint32_t *list, uint32_t n, uint32_t *stamp,
                        uint32_t tag, uint32_t *out, uint32_t cap);
/* partitioned mode: ids of another rank's expansion claimed into out (have: entries so far) */
uint32_t amgd_fs_claim_ext(const uint32_t *ids, uint64_t n, uint32_t *stamp, uint32_t tag, uint32_t *out,
                           uint32_t have, uint32_t cap);
uint8_t *amgd_bad_rows(const dcsr *ns, uint32_t *nbad);
uint64_t amgd_expand_pick(const dcsr *Xf, const uint8_t *bad, uint32_t **pi, uint32_t **pj);
void amgd_skel_binarize(dcsr *A, int mode);
void amgd_scale_diag_match(dcsr *W, const double *v, const double *wuc);
void amgd_csc_gemv(const dcsr *Rt, const uint64_t *perm, const double *a, const double *x,
                   double *z);
/* misc vector kernels */
void amgd_vdiv_guard(double *r, const double *num, const double *den, uint64_t n); /* r=num/den, 0 where den==0 */
void amgd_alpha_update(double *alpha, const double *Dc, const double *w2, uint64_t n);
void amgd_u8_not(const uint8_t *a, uint8_t *b, uint64_t n);
void amgd_u8_nonzero(const double *a, uint8_t *m, uint64_t n);
uint64_t amgd_u8_count(const uint8_t *m, uint64_t n);
void amgd_vcompact(double *dst, const double *src, const uint8_t *mask, uint64_t n);
void amgd_vexpand_add(double *dst, const double *src, const uint8_t *mask, uint64_t n);
void amgd_vzero_where(double *a, const uint8_t *mask_keep, uint64_t n);
void amgd_ids_iota(unsigned long *id, uint64_t n);
/* one Chebyshev update of the V-cycle's composed path (amg.c:155, :164):
   cn = beta*(c + D.*r) [- gamma*cn], cn holding c_{i-1} on entry when has_prev */
void amgd_vc_cheb_update(double *cn, const double *c, const double *D, const double *r, double beta,
                         double gamma, int has_prev, uint64_t n);

/* ---------------- V-cycle (amgd_solve.hip; driver amgd_vcycle.c) ---------------- */
void amgd_vc_remap_cols(const uint32_t *col, uint64_t nnz, const uint32_t *pos_next, uint32_t off_next,
                        uint32_t *out);                         /* out = pos_next[col] - off_next */
void amgd_vc_scatter(double *b, const double *db, const uint32_t *pos, uint64_t n);   /* b[pos[i]] = db[i] */
/* dx[i] = x[pos[i]] (sub: - avg) */
void amgd_vc_gather(double *dx, const double *x, const uint32_t *pos, uint64_t n, int sub, double avg);
/* the three operations of a level, each one kernel over a row-sum policy (amgd_vc_dev.h).
   fam: 0 the short-row policies (a block per 256 rows), 1 the long-row ones (a wavefront per
   row group).  K == 1: one vector; K = 2 / 4 / 8: interleaved right-hand sides, element
   (position q, column j) at q*K + j -- same expressions, same bits per column.
   b += Wt bF (map NULL: b is the coarse slice; else, K == 1 only, row c writes b[map[c]]: a
   rank's own C rows in the partitioned cycle);
   xf = W xc, bf -= AfP xc, c = D.*bf (add: xf += c);
   cn = beta*(c + D.*(bf - Af cg)) [- gamma*cn] (xf != NULL: xf += cn), cg the vector the row
   sums gather from (Af's columns index it) and c, cn, bf, D, xf at the rows' own entries: one
   GPU passes cg == c, a rank's row block the whole c and the rest offset to its rows.
   K > 1 has neither a map nor a separate cg: either is refused (amgd_set_error, no launch) */
void amgd_vc_restrict(int fam, int K, const dcsr *Wt, const double *bF, double *b, const uint32_t *map);
void amgd_vc_prolong(int fam, int K, const dcsr *W, const dcsr *AfP, const double *D, const double *xc,
                     double *xf, double *bf, double *c, int add);
void amgd_vc_cheb(int fam, int K, const dcsr *Af, const double *D, const double *bf, const double *cg,
                  const double *c, double *cn, double beta, double gamma, int has_prev, double *xf);
/* the coarse tail: levels of at most AMGD_VC_TAIL_ROWS positions together, one workgroup */
#define AMGD_VC_TAIL_ROWS 1024
#define AMGD_VC_MAXSTEPS 16
typedef struct {
  const uint64_t *wt_ro, *w_ro, *p_ro, *af_ro;
  const uint32_t *wt_col, *w_col, *p_col, *af_col;
  const double *wt_a, *w_a, *p_a, *af_a, *D;
  uint32_t nf, nc, off, steps;                 /* steps = m - 1 Chebyshev updates */
  double beta[AMGD_VC_MAXSTEPS], gamma[AMGD_VC_MAXSTEPS];
} amgd_vc_tlev;
/* lv: nl descriptors on the device, finest first; up_only: no restriction, no bottom solve */
void amgd_vc_tail(const amgd_vc_tlev *lv, int nl, double *b, double *x, double *c0, double *c1,
                  uint32_t N, double dbot, int up_only);
/* partitioned cycle (amgd_vcycle.c): b[map[c]] += t[c], the composed restriction's second half
   on a rank's own C rows */
void amgd_vc_add_map(double *b, const uint32_t *map, const double *t, uint64_t n);
/* halo exchange: buf[k] = v[idx[k]] before the alltoallv, v[idx[k]] = buf[k] after it */
void amgd_vc_pack(double *buf, const double *v, const uint32_t *idx, uint64_t n);
void amgd_vc_unpack(double *v, const uint32_t *idx, const double *buf, uint64_t n);
/* out[i] = ((+0 + seg[0][i]) + seg[1][i]) + ... with seg[r] = segs + r*n (crs_solve's b in rank order) */
void amgd_vc_rank_sum(double *out, const double *segs, int nr, uint64_t n);
/* a group's columns: up to 8 pointers, passed to a kernel by value (entries >= K: NULL) */
typedef struct { const double *p[8]; } amgd_cptr8;
typedef struct { double *p[8]; } amgd_ptr8;
/* the K columns base + j*ld */
static inline amgd_cptr8 amgd_cptr8_strided(const double *base, uint64_t ld, int K) {
  amgd_cptr8 t;
  for (int j = 0; j < 8; j++) t.p[j] = j < K ? base + (uint64_t)j * ld : 0;
  return t;
}
static inline amgd_ptr8 amgd_ptr8_strided(double *base, uint64_t ld, int K) {
  amgd_ptr8 t;
  for (int j = 0; j < 8; j++) t.p[j] = j < K ? base + (uint64_t)j * ld : 0;
  return t;
}
/* the K columns p[0 .. K) */
static inline amgd_cptr8 amgd_cptr8_of(const double *const *p, int K) {
  amgd_cptr8 t;
  for (int j = 0; j < 8; j++) t.p[j] = j < K ? p[j] : 0;
  return t;
}
static inline amgd_ptr8 amgd_ptr8_of(double *const *p, int K) {
  amgd_ptr8 t;
  for (int j = 0; j < 8; j++) t.p[j] = j < K ? p[j] : 0;
  return t;
}
/* K = 2 / 4 / 8 interleaved right-hand sides (amgd_solve_mrhs.hip), into and out of the
   layout: b[pos[i]*K + j] = in->p[j][i]; out->p[j][i] =
   x[pos[i]*K + j] (- avg[j], host, when sub); pos NULL: the identity */
void amgd_vcn_scatter(double *b, const amgd_cptr8 *in, const uint32_t *pos, uint64_t n, int K);
void amgd_vcn_gather(const amgd_ptr8 *out, const double *x, const uint32_t *pos, uint64_t n, int K, int sub,
                     const double *avg);
/* x[j] = dbot*b[j], j < K.  out[q] = x[q*K + j] */
void amgd_vcn_bottom(double *x, const double *b, double dbot, int K);
void amgd_vcn_col(double *out, const double *x, uint64_t n, int K, int j);
void amgd_vcn_putcol(double *x, const double *in, uint64_t n, int K, int j);   /* x[q*K + j] = in[q] */
/* ---------------- flexible GMRES (amgd_krylov.hip; driver amgd_krylov.c) ---------------- */
/* basis blocks are column-major, vector t at V + t*ld.  d[t] = v_t . w for t < nb, every sum
   in a fixed order (part: nb * amgd_kry_grid(n) doubles); prev != NULL: hsum[t] = prev[t] + d[t] */
int amgd_kry_tile(void);                /* vectors per workgroup row of the multi-dot */
int amgd_kry_grid(uint64_t n);
void amgd_kry_mdot(const double *V, uint64_t ld, const double *w, uint64_t n, int nb, double *part, double *d,
                   const double *prev, double *hsum);
/* w = ((w - c_0 v_0) - c_1 v_1) ... (add: +), c on the device; nrm2 != NULL: nrm2[0] = sum of
   the new w's squares, root[0] = its square root (part: amgd_kry_grid(n) doubles) */
void amgd_kry_axpys(double *w, const double *V, uint64_t ld, const double *c, int nb, uint64_t n, int add,
                    double *part, double *nrm2, double *root);
void amgd_kry_scale(double *v, const double *w, const double *h, uint64_t n);   /* v = w / h[0] */
/* the ranks' partial sums combined in rank order (a row-partitioned hierarchy): g holds rank
   r's nb sums at g + r*nb; out[t] = (g_0[t] + g_1[t]) + ... + g_{np-1}[t]; prev != NULL:
   hsum[t] = prev[t] + out[t]; root != NULL: root[0] = sqrt(out[0]) -- what k_kry_fin applies */
void amgd_kry_comb(const double *g, int np, int nb, double *out, const double *prev, double *hsum, double *root);
/* ---- several right-hand sides in lock-step (amgd_krylov_device_n) ---- */
/* the K-column level-0 product (amgd_krylov_mrhs.hip), K = 2 / 4 / 8: z_j = alpha*y_j + beta*(A x_j)
   (alpha == 0 or y NULL: beta*(A x_j)), every (row, column) value bit for bit amgd_spmv's.  xi: K*A->cn
   doubles, receives the operands interleaved (one copy per product); fam 0 the short-row, 1 the
   long-row kernel.  A row of A may have any length here; the driver keeps outlier-row matrices out */
void amgd_kry_spmv_n(const dcsr *A, int K, int fam, const amgd_cptr8 *x, const amgd_ptr8 *z, double alpha,
                     const amgd_cptr8 *y, double beta, double *xi);
/* the orthogonalisation kernels for nc <= 8 columns in one launch each: column q has its own
   basis, w, coefficients and partial blocks; the paired / unpaired form is chosen per column
   from its own pointers, the grid and the tile loop are the single forms' */
typedef struct {
  const double *V;       /* basis block, vector t at V + t*ld */
  double *w;
  int nb;
  double *part;          /* nb * amgd_kry_grid(n) doubles */
  double *d;             /* mdot: the nb dots; axpys: the coefficients (read) */
  const double *prev;    /* mdot: NULL, or hsum[t] = prev[t] + d[t] */
  double *hsum;
  double *nrm2, *root;   /* axpys: NULL, or the sum of the new w's squares and its root */
  double *vout;          /* scale: vout = w / h[0] */
  const double *h;
} amgd_kry_col;
void amgd_kry_mdot_n(const amgd_kry_col *c, int nc, uint64_t ld, uint64_t n);
void amgd_kry_axpys_n(const amgd_kry_col *c, int nc, uint64_t ld, uint64_t n);
void amgd_kry_scale_n(const amgd_kry_col *c, int nc, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif
