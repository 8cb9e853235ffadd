/*
 * amgd_drv.h -- what the one-GPU driver (amgd_setup.c) and the row-partitioned driver
 * (amgd_psetup.c) share (amgd_drv.c): the small helpers, the transposed-product rule, the
 * coarsening set-up, Lanczos / PCG over an operator record, the hierarchy with its export
 * and frees, and the per-setup statistics.  Each driver keeps only what really differs:
 * its level loop and the routines that work on its matrix type.
 */
#ifndef AMGD_DRV_H
#define AMGD_DRV_H
#include <stdint.h>

#include "amg_setup.h"
#include "amgd.h"
#include "amgd_part.h"
#include "omp_amg_amd.h"

static inline double *dalloc(uint64_t n) { return (double *)amgd_alloc_f64(n * 8 + 8); }
static inline double *dones(uint64_t n) { double *p = dalloc(n); amgd_vfill(p, n, 1.0); return p; }
static inline double *dzeros(uint64_t n) { double *p = dalloc(n); amgd_vfill(p, n, 0.0); return p; }
static inline void add_time(double *acc, double *t0) {
  amgd_sync();
  double t = amgd_wtime();
  *acc += (t - *t0) * 1e3;
  *t0 = t;
}
int amgd_verbose(int rank);              /* AMGD_VERBOSE=1, on rank 0 only */
int amgd_phases_on(void);                /* AMGD_PHASES=1 */

/* per-setup statistics: begin zeroes *st and every counter a setup reads (SpMV / SpGEMM
   bytes, timers, pool peak, per-call module state, the UB count); end fills the counter
   fields.  amgd_ub_note records a reference-undefined event (non-termination) in the stats
   begun last -- site 1 find_support theta -> 0, 2 a one-row R, 3 a sweep that removed
   nothing, 4 the selection count past nnz(R) + nc, 5 the interpolation loop's skeleton
   stalled (amg_setup.c:1316-1330, :700-860); the first AMGD_UB_LOG keep site and level */
void amgd_drv_stats_begin(amgd_stats *st);
void amgd_drv_stats_end(amgd_stats *st);
void amgd_ub_note(int site, int level);

/* X = A*B runs as (B'A')' when A' has long rows: mean row of A' >= 64 and at least twice
   B's (local or global counts; zero-row operands: never) */
int amgd_via_t(uint64_t nnz_At, uint32_t rows_At, uint64_t nnz_B, uint32_t rows_B);

/* coarsening: one buffer per stage of the sweep (amgd_coarsen.hip) */
typedef struct {
  uint8_t *vf, *ma, *mb;
  double *vfd, *g, *w1, *w2a, *w2, *w, *x1, *x2, *m1, *m2, *amax;
  uint32_t *anyvc, *stamp, *front[2], *cnt[2];
} amgd_cs_work;
void amgd_cs_work_init(amgd_cs_work *k, uint32_t n, uint8_t *vc);   /* vc = 0, vf = 1 */
void amgd_cs_work_free(amgd_cs_work *k);
/* incremental sweeps (AMGD_CS_INC, AMGD_CS_MIN_ROWS, short rows), one thread per listed row
   (AMGD_CS_LIST_NNZ), the dirty-set limit */
typedef struct { int inc, list_mode; uint32_t limit; } amgd_cs_rule;
amgd_cs_rule amgd_cs_rule_of(uint32_t n, uint64_t nnz_S, uint64_t nnz_St);
/* w = (1./w1).*w2; mask1 = w > ctol^2; x1 = mask1.*g; 1 when the norm bound is met (the
   sweep loop ends; a level with no C point gets the row of max(w1)) */
int amgd_cs_bound_met(const amgd_cs_work *k, uint32_t n, double ctol, uint8_t *vc,
                      const amgd_csrows *rows, int it, int say);

/* a square operator, for the Krylov routines */
typedef struct {
  uint32_t n;                 /* square: rows = cols */
  const void *A;
  void (*spmv)(const void *A, const double *x, double *z);   /* z = A*x, whole vectors */
  double (*fro_minus_eye)(const void *A);
  double (*a00)(const void *A);                               /* value of a 1 x 1 matrix */
} amgd_linop;
/* Lanczos + tdeig (amg_setup.c:2435-2726), tdeig on the host: the eigenvalue estimates */
uint32_t amgd_lanczos(const amgd_linop *A, double *out);
/* the smoother's scalars from Lanczos on DAD: returns the scale 2/(a+b) of D, sets rho and
   the Chebyshev degree m (chebsim, amg_setup.c:2412) */
double amgd_cheb_fit(const amgd_linop *DAD, double gamma2, double *rho, double *m);
/* PCG (amg_setup.c:2242): z = M.*r, at most min(n,100) iterations; r is overwritten */
typedef struct { uint32_t its; double rho, rho_stop; } amgd_pcg_info;
amgd_pcg_info amgd_pcg(double *x, const amgd_linop *A, double *r, const double *M, double tol, const double *b);

/* the hierarchy, whole (one GPU: d) or this rank's row blocks (partitioned: p) */
typedef union { dcsr *d; pmat *p; } amgd_mat;
typedef struct {
  amgd_mat A, Af, W, AfP;
  uint8_t *vc;                 /* whole vectors in either mode */
  double *D;                   /* F points */
  unsigned long *idc, *idf;
  double m, rho;
  apart *Pn, *Pf;              /* partitioned: rows of A (owned by this level), F points */
} amgd_level;
struct amgd_hier {
  int part;                    /* 1: partitioned */
  uint32_t nlevels, cap, n0;
  amgd_level *lv;
  unsigned long *id;           /* device, level-0 ids 1..n */
  int nullspace;
  double tolc, gamma;
  struct amgd_vc_plan *plan;   /* the V-cycle's plan, built on the first solve (amgd_vcycle.c) */
  struct amgd_kry_ws *kry;     /* the Krylov workspace kept with the plan (amgd_krylov.c) */
  struct amgd_kry_nws *kryn;   /* the slots of amgd_krylov_device_n (amgd_krylov.c) */
};
amgd_hier *amgd_hier_new(int part);
amgd_level *amgd_hier_level(amgd_hier *h, uint32_t l);    /* grows the level array */
/* after an unwound (out-of-HBM) setup: the host side of a partial hierarchy */
void amgd_hier_free_host(amgd_hier **h);
/* the solve plan of a hierarchy (amgd_vcycle.c): free with its device blocks / its host side only */
void amgd_vc_plan_free(struct amgd_vc_plan **p);
void amgd_vc_plan_free_host(struct amgd_vc_plan **p);
/* the plan and its tail built, each in its own amgd_try: 0, -1 bad hierarchy, -2 out of HBM */
int amgd_vc_prepare(amgd_hier *h);
/* the Krylov workspace of a hierarchy (amgd_krylov.c): with its device blocks / host side only */
void amgd_kry_ws_free(struct amgd_kry_ws **w);
void amgd_kry_ws_free_host(struct amgd_kry_ws **w);
void amgd_kry_nws_free(struct amgd_kry_nws **w);
void amgd_kry_nws_free_host(struct amgd_kry_nws **w);
#endif
