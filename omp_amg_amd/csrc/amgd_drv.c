/*
 * amgd_drv.c -- the core shared by the one-GPU and the partitioned setup drivers
 * (amgd_drv.h): everything that is the same in both level loops lives here once.
 *
 * Compiled with -ffp-contract=off so host arithmetic (chebsim, tdeig, threshold
 * expressions) rounds exactly like the reference's ISO-C build.
 */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "amgd_drv.h"
#include "amgd_hostmath.h"

#define API __attribute__((visibility("default")))

int amgd_verbose(int rank) { return amgd_knob(AMGD_K_VERBOSE) && rank == 0; }

/* ------------------------------------------------------------------------ */
/* statistics                                                                */
/* ------------------------------------------------------------------------ */
extern uint64_t amgd_spmv_bytes(void);
extern uint64_t amgd_spmv_bytes_strict(void);
extern uint64_t amgd_spmv_launches(void);
extern uint64_t amgd_spgemm_launches(void);
extern void amgd_spmv_bytes_reset(void);
extern void amgd_spmv_rw_counts(uint64_t *bytes, uint64_t *launches);
extern void amgd_spgemm_bytes_reset(void);
extern uint64_t amgd_spgemm_bytes(void);

static amgd_stats *g_st;               /* the stats being filled */
static uint64_t g_ub;                  /* reference-undefined events of this setup */
void amgd_ub_note(int site, int level) {
  if (g_ub < AMGD_UB_LOG) { g_st->ub_site[g_ub] = (uint8_t)site; g_st->ub_level[g_ub] = (uint8_t)level; }
  g_ub++;
}
void amgd_drv_stats_begin(amgd_stats *st) {
  memset(st, 0, sizeof *st);
  g_st = st;
  g_ub = 0;
  amgd_knobs_read_env();                /* the switches' variables, once per setup */
  amgd_reset_call_state();
  amgd_pool_peak_reset();               /* amgd_stats.peak_bytes: this setup's peak */
  amgd_timer_reset();
  amgd_spmv_bytes_reset();
  amgd_spgemm_bytes_reset();
}
void amgd_drv_stats_end(amgd_stats *st) {
  st->rap_kernel_ms = amgd_timer_ms(0);
  st->spmv_kernel_ms = amgd_timer_ms(1);
  st->spmv_bytes = amgd_spmv_bytes();
  st->spmv_bytes_strict = amgd_spmv_bytes_strict();
  st->spmv_launches = amgd_spmv_launches();
  st->rap_launches = amgd_spgemm_launches();
  st->rap_bytes = amgd_spgemm_bytes();
  amgd_spmv_rw_counts(st->spmv_rw_bytes_strict, st->spmv_rw_launches);
  for (int i = 0; i < 3; i++) st->spmv_rw_ms[i] = amgd_timer_ms(2 + i);
  amgd_spmv_bytes_reset();
  amgd_spgemm_bytes_reset();
  st->ub_events = (uint32_t)g_ub;
  st->peak_bytes = amgd_pool_peak_bytes();
}

/* phase profile (AMGD_PHASES=1): device-synchronised time per (level, phase),
   printed at the end of the setup; costs one stream sync per mark. */
static const char *ph_name[PH_N] = {"coarsen", "smoother", "interp0", "qfactor", "W0", "S_pat",
                                    "lmop", "pcg", "W", "AfW", "R", "fs_setup", "fs_spmv",
                                    "fs_max", "fs_sel", "expand", "exp_R0", "final", "rap"};
#define PH_MAXL 64
static double g_ph[PH_MAXL][PH_N], g_ph_t;
static double g_phpk[PH_MAXL][PH_N];      /* GB: pool peak inside the phase */
int amgd_phases_on(void) { return amgd_knob(AMGD_K_PHASES) != 0; }
void amgd_ph_mark(int lvl, int id) {
  if (!amgd_phases_on()) return;
  amgd_sync();
  double t = amgd_wtime();
  const double pk = amgd_pool_ipeak_take() / 1e9;
  if (id >= 0 && lvl >= 0 && lvl < PH_MAXL) {
    g_ph[lvl][id] += (t - g_ph_t) * 1e3;
    if (pk > g_phpk[lvl][id]) g_phpk[lvl][id] = pk;
  }
  g_ph_t = t;
}
void amgd_ph_report(uint32_t nl) {
  if (!amgd_phases_on()) return;
  double tot[PH_N] = {0};
  fprintf(stderr, "phase ms per level:\nlvl");
  for (int p = 0; p < PH_N; p++) fprintf(stderr, " %9s", ph_name[p]);
  fprintf(stderr, "\n");
  for (uint32_t l = 0; l < nl && l < PH_MAXL; l++) {
    fprintf(stderr, "%3u", l);
    for (int p = 0; p < PH_N; p++) { fprintf(stderr, " %9.1f", g_ph[l][p]); tot[p] += g_ph[l][p]; }
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "sum");
  for (int p = 0; p < PH_N; p++) fprintf(stderr, " %9.1f", tot[p]);
  fprintf(stderr, "\nphase peak GB (pool in use, max inside the phase):\nlvl");
  for (int p = 0; p < PH_N; p++) fprintf(stderr, " %9s", ph_name[p]);
  fprintf(stderr, "\n");
  for (uint32_t l = 0; l < nl && l < PH_MAXL; l++) {
    fprintf(stderr, "%3u", l);
    for (int p = 0; p < PH_N; p++) fprintf(stderr, " %9.2f", g_phpk[l][p]);
    fprintf(stderr, "\n");
  }
  uint64_t nm, nr;
  double gb, ms;
  amgd_pool_stats(&nm, &gb, &ms, &nr);
  fprintf(stderr, "pool: %lu driver allocations, %.1f GB, %.1f ms in hipMalloc, %lu cache flushes\n",
          (unsigned long)nm, gb, ms, (unsigned long)nr);
  memset(g_ph, 0, sizeof g_ph);
  memset(g_phpk, 0, sizeof g_phpk);
}

int amgd_via_t(uint64_t nnz_At, uint32_t rows_At, uint64_t nnz_B, uint32_t rows_B) {
  const uint64_t avg_at = rows_At ? nnz_At / rows_At : 0, avg_b = rows_B ? nnz_B / rows_B : 0;
  return avg_at >= 64 && avg_at >= 2 * avg_b;
}

/* ------------------------------------------------------------------------ */
/* coarsen (amg_setup.c:2737): what the two sweep loops share                */
/* ------------------------------------------------------------------------ */
void amgd_cs_work_init(amgd_cs_work *k, uint32_t n, uint8_t *vc) {
  k->vf = (uint8_t *)amgd_alloc(n + 1); k->ma = (uint8_t *)amgd_alloc(n + 1);
  k->mb = (uint8_t *)amgd_alloc(n + 1);
  k->vfd = dones(n); k->g = dalloc(n); k->w1 = dalloc(n); k->w2a = dalloc(n); k->w2 = dalloc(n);
  k->w = dalloc(n); k->x1 = dalloc(n); k->x2 = dalloc(n); k->m1 = dalloc(n); k->m2 = dalloc(n);
  k->amax = dalloc(n);
  k->anyvc = (uint32_t *)amgd_alloc(4);
  k->stamp = (uint32_t *)amgd_alloc(4ull * n + 4);
  for (int q = 0; q < 2; q++) {
    k->front[q] = (uint32_t *)amgd_alloc(4ull * n + 4);
    k->cnt[q] = (uint32_t *)amgd_alloc(64);
  }
  amgd_memset(vc, 0, n);
  amgd_memset(k->vf, 1, n);
  amgd_memset(k->anyvc, 0, 4);
  amgd_memset(k->stamp, 0, 4ull * n);
  amgd_memset(k->cnt[0], 0, 64);
}
void amgd_cs_work_free(amgd_cs_work *k) {
  amgd_free(k->vf); amgd_free(k->ma); amgd_free(k->mb); amgd_free(k->vfd); amgd_free(k->g);
  amgd_free(k->w1); amgd_free(k->w2a); amgd_free(k->w2); amgd_free(k->w); amgd_free(k->x1);
  amgd_free(k->x2); amgd_free(k->m1); amgd_free(k->m2); amgd_free(k->amax); amgd_free(k->anyvc);
  amgd_free(k->stamp);
  for (int q = 0; q < 2; q++) { amgd_free(k->front[q]); amgd_free(k->cnt[q]); }
}
amgd_cs_rule amgd_cs_rule_of(uint32_t n, uint64_t nnz_S, uint64_t nnz_St) {
  const uint64_t min_rows = (uint64_t)amgd_knob(AMGD_K_CS_MIN_ROWS);
  amgd_cs_rule r;
  r.inc = amgd_knob(AMGD_K_CS_INC) != 0 && n >= min_rows && nnz_S + nnz_St <= 64ull * n;
  /* very short rows: one thread per listed row (list mode) beats the block filter */
  r.list_mode = nnz_S <= (uint64_t)amgd_knob(AMGD_K_CS_LIST_NNZ) * n;
  r.limit = n / 4;
  return r;
}
int amgd_cs_bound_met(const amgd_cs_work *k, uint32_t n, double ctol, uint8_t *vc,
                      const amgd_csrows *rows, int it, int say) {
  amgd_cs_w_mask1(n, k->w1, k->w2, k->w, ctol * ctol, k->g, k->ma, k->x1, rows, 4);
  uint64_t mi = 0;
  double wm = 0;
  double w1m = amgd_max_first2(k->w1, k->w, n, &mi, &wm);    /* max(w1) (first index), max(w) */
  double b = (w1m < wm) ? sqrt(w1m) : sqrt(wm);
  if (!(b <= ctol)) return 0;
  uint32_t any = 0;
  amgd_d2h(&any, k->anyvc, 4);
  if (!any) { uint8_t one = 1; amgd_h2d(vc + mi, &one, 1); }
  if (say) printf("  coarsen: %d sweeps, norm bound = %f\n", it, b);
  return 1;
}

/* ------------------------------------------------------------------------ */
/* Lanczos + tdeig (amg_setup.c:2435-2726), PCG (amg_setup.c:2242)           */
/* ------------------------------------------------------------------------ */
#define KMAX 299
uint32_t amgd_lanczos(const amgd_linop *A, double *out) {
  const uint32_t rn = A->n;
  /* start vector: libc rand()/RAND_MAX, like the reference (amg_setup.c:2445-2448),
     so the process-wide rand() stream advances identically */
  double *rh = (double *)malloc((size_t)rn * 8 + 8);
  for (uint32_t i = 0; i < rn; i++) rh[i] = (double)rand() / (double)RAND_MAX;
  double *r = dalloc(rn);
  amgd_h2d(r, rh, (size_t)rn * 8);
  free(rh);
  double l[KMAX + 2], y[KMAX + 2], d[KMAX + 2], v[KMAX + 2];
  double beta = amgd_norm2(r, rn), beta2 = beta * beta, change;
  beta = sqrt(beta2);
  uint32_t k = 0;
  {
    double fr = A->fro_minus_eye(A->A), fro = sqrt(fr), fro2 = fro * fro;
    fro = sqrt(fro2);
    if (fro < 1e-11) { l[0] = 1; l[1] = 1; y[0] = 0; y[1] = 0; k = 2; change = 0.0; }
    else change = 1.0;
  }
  if (rn == 1) {
    const double a00 = A->a00(A->A);
    l[0] = a00; l[1] = a00; y[0] = 0; y[1] = 0; k = 2; change = 0.0;
  }
  double *qk = dzeros(rn), *qkm1 = dalloc(rn), *Aqk = dalloc(rn);
  while (k < KMAX && (change > 1e-5 || y[0] > 1e-3 || y[k - 1] > 1e-3)) {
    k++;
    amgd_lanczos_step(r, 1. / beta, qk, qkm1, rn);           /* qkm1 = qk; qk = r/beta */
    A->spmv(A->A, qk, Aqk);
    double alpha = amgd_dot(qk, Aqk, rn);
    amgd_lanczos_resid(r, Aqk, qk, alpha, qkm1, beta, rn);    /* r = Aqk - a qk - b qkm1 */
    if (k == 1) { l[0] = alpha; y[0] = 1; }
    else {
      double l0 = l[0], lkm2 = l[k - 2];
      d[0] = 0;
      for (uint32_t i = 1; i < k; i++) d[i] = l[i - 1];
      d[k] = 0;
      v[0] = alpha;
      for (uint32_t i = 1; i < k; i++) v[i] = beta * y[i - 1];
      tdeig(l, y, d, v, (int)k - 1);
      change = fabs(l0 - l[0]) + fabs(lkm2 - l[k - 1]);
    }
    beta = amgd_norm2(r, rn);
    beta2 = beta * beta;
    beta = sqrt(beta2);
    if (beta == 0) break;
  }
  uint32_t n = 0;
  for (uint32_t i = 0; i < k; i++) if (y[i] < 0.01) out[n++] = l[i];
  amgd_free(r); amgd_free(qk); amgd_free(qkm1); amgd_free(Aqk);
  return n;
}

double amgd_cheb_fit(const amgd_linop *DAD, double gamma2, double *rho, double *m) {
  double lambda[KMAX + 2], c;
  const uint32_t k = amgd_lanczos(DAD, lambda);
  const double a = lambda[0], b = lambda[k - 1];
  *rho = (b - a) / (b + a);
  chebsim(m, &c, *rho, gamma2);
  return 2. / (a + b);
}

amgd_pcg_info amgd_pcg(double *x, const amgd_linop *A, double *r, const double *M, double tol, const double *b) {
  const uint32_t rn = A->n;
  amgd_pcg_info info = {0, 0, 0};
  amgd_vfill(x, rn, 0.0);
  if (rn == 0) return info;
  double *p = dzeros(rn), *z = dalloc(rn), *w = dalloc(rn);
  amgd_vmul_dot_prep(z, M, r, rn);
  double rho = amgd_dot(r, z, rn);
  double rho_0 = amgd_dot3(M, b, rn);
  double rho_stop = tol * tol * rho_0, rho_old = 1, alpha, beta;
  uint32_t n = rn <= 100 ? rn : 100, k = 0;
  while (rho > rho_stop && k < n) {
    k++;
    beta = rho / rho_old;
    amgd_pcg_p(p, z, beta, rn);                  /* p = p*beta + z */
    A->spmv(A->A, p, w);
    alpha = amgd_dot(p, w, rn);
    alpha = rho / alpha;
    amgd_pcg_xrz(x, r, z, p, w, M, alpha, rn);   /* x += p*a; r -= w*a; z = M.*r */
    rho_old = rho;
    rho = amgd_dot(r, z, rn);
  }
  info.its = k;
  info.rho = rho;
  info.rho_stop = rho_stop;
  amgd_free(p); amgd_free(z); amgd_free(w);
  return info;
}

/* ------------------------------------------------------------------------ */
/* hierarchy                                                                 */
/* ------------------------------------------------------------------------ */
amgd_hier *amgd_hier_new(int part) {
  amgd_hier *h = (amgd_hier *)calloc(1, sizeof(amgd_hier));
  h->part = part;
  h->cap = 64;
  h->lv = (amgd_level *)calloc(h->cap, sizeof(amgd_level));
  return h;
}
amgd_level *amgd_hier_level(amgd_hier *h, uint32_t l) {
  if (l + 1 >= h->cap) {
    h->cap *= 2;
    h->lv = (amgd_level *)realloc(h->lv, h->cap * sizeof(amgd_level));
    memset(h->lv + h->cap / 2, 0, (h->cap / 2) * sizeof(amgd_level));
  }
  return &h->lv[l];
}

/* the three things that differ by mode, per matrix: to the host (partitioned: gathered,
   every rank gets the whole), free, free of the host headers only */
static struct csr_mat *mat_to_host(const amgd_hier *h, amgd_mat A) {
  dcsr *F = h->part ? pm_gather_full(A.p) : A.d;
  struct csr_mat *M = (struct csr_mat *)malloc(sizeof *M);
  M->rn = F->rn;
  M->cn = F->cn;
  M->row_off = (amg_uint *)malloc(((size_t)F->rn + 1) * sizeof(amg_uint));
  M->col = (amg_uint *)malloc((F->nnz ? F->nnz : 1) * sizeof(amg_uint));
  M->a = (double *)malloc((F->nnz ? F->nnz : 1) * sizeof(double));
  amgd_to_host_cols(F, M->row_off, M->col, M->a);
  if (h->part) dcsr_free(&F);
  return M;
}
static void mat_free(const amgd_hier *h, amgd_mat *A) {
  if (h->part) pm_free(&A->p);
  else dcsr_free(&A->d);
}
static void mat_free_host(const amgd_hier *h, amgd_mat *A) {
  if (h->part) { if (A->p) free(A->p->m); free(A->p); A->p = NULL; }
  else { free(A->d); A->d = NULL; }
}
static double host_nnz(const struct csr_mat *M) { return (double)M->row_off[M->rn]; }

API int amgd_hier_export(const amgd_hier *h, struct amg_setup_data *data) {
  amgd_sync();
  double t0 = amgd_wtime();
  uint32_t nl = h->nlevels, cap = nl + 1;
  data->tolc = h->tolc;
  data->gamma = h->gamma;
  data->n = (double *)malloc(cap * 8); data->nnz = (double *)malloc(cap * 8);
  data->nnzf = (double *)malloc(cap * 8); data->nnzfp = (double *)malloc(cap * 8);
  data->m = (double *)malloc(cap * 8); data->rho = (double *)malloc(cap * 8);
  data->A = (struct csr_mat **)malloc(cap * sizeof(void *));
  data->Af = (struct csr_mat **)malloc(cap * sizeof(void *));
  data->W = (struct csr_mat **)malloc(cap * sizeof(void *));
  data->AfP = (struct csr_mat **)malloc(cap * sizeof(void *));
  data->idc = (amg_uint **)malloc(cap * sizeof(void *));
  data->idf = (amg_uint **)malloc(cap * sizeof(void *));
  data->C = (double **)malloc(cap * sizeof(void *));
  data->F = (double **)malloc(cap * sizeof(void *));
  data->D = (double **)malloc(cap * sizeof(void *));
  data->id = (amg_uint *)malloc((size_t)h->n0 * sizeof(amg_uint) + 8);
  amgd_d2h(data->id, h->id, (size_t)h->n0 * 8);
  for (uint32_t l = 0; l < nl; l++) {
    const amgd_level *L = &h->lv[l];
    data->A[l] = mat_to_host(h, L->A);
    data->n[l] = data->A[l]->cn;
    data->nnz[l] = host_nnz(data->A[l]);
    if (l + 1 == nl) break;
    uint32_t rn = data->A[l]->rn, rnf = h->part ? L->Pf->n : L->Af.d->rn, rnc = rn - rnf;
    uint8_t *vc = (uint8_t *)malloc(rn + 1);
    amgd_d2h(vc, L->vc, rn);
    data->C[l] = (double *)malloc((size_t)rn * 8 + 8);
    data->F[l] = (double *)malloc((size_t)rn * 8 + 8);
    for (uint32_t i = 0; i < rn; i++) { data->C[l][i] = vc[i] ? 1. : 0.; data->F[l][i] = vc[i] ? 0. : 1.; }
    free(vc);
    data->D[l] = (double *)malloc((size_t)rnf * 8 + 8);
    amgd_d2h(data->D[l], L->D, (size_t)rnf * 8);
    data->m[l] = L->m;
    data->rho[l] = L->rho;
    data->Af[l] = mat_to_host(h, L->Af);
    data->W[l] = mat_to_host(h, L->W);
    data->AfP[l] = mat_to_host(h, L->AfP);
    data->nnzf[l] = host_nnz(data->Af[l]);
    data->nnzfp[l] = host_nnz(data->AfP[l]);
    data->idc[l] = (amg_uint *)malloc((size_t)rnc * 8 + 8);
    data->idf[l] = (amg_uint *)malloc((size_t)rnf * 8 + 8);
    amgd_d2h(data->idc[l], L->idc, (size_t)rnc * 8);
    amgd_d2h(data->idf[l], L->idf, (size_t)rnf * 8);
  }
  data->nlevels = nl;
  data->nullspace = (amg_uint)h->nullspace;
  if (g_st) g_st->t_copy_ms = (amgd_wtime() - t0) * 1e3;
  return 0;
}

API void amgd_hier_free(amgd_hier **hp) {
  amgd_hier *h = *hp;
  if (!h) return;
  for (uint32_t l = 0; l < h->nlevels; l++) {
    amgd_level *L = &h->lv[l];
    mat_free(h, &L->A); mat_free(h, &L->Af); mat_free(h, &L->W); mat_free(h, &L->AfP);
    if (L->vc) amgd_free(L->vc);
    if (L->D) amgd_free(L->D);
    if (L->idc) amgd_free(L->idc);
    if (L->idf) amgd_free(L->idf);
    apart_free(&L->Pn);
    apart_free(&L->Pf);
  }
  if (h->id) amgd_free(h->id);
  amgd_vc_plan_free(&h->plan);
  amgd_kry_ws_free(&h->kry);
  amgd_kry_nws_free(&h->kryn);
  free(h->lv);
  free(h);
  *hp = NULL;
}

/* Its device blocks were released by the unwind already (amgd_try), so nothing here
   touches the device pool: matrix headers, partitions, the level array. */
void amgd_hier_free_host(amgd_hier **hp) {
  amgd_hier *h = *hp;
  if (!h) return;
  for (uint32_t l = 0; l < h->cap; l++) {
    amgd_level *L = &h->lv[l];
    mat_free_host(h, &L->A); mat_free_host(h, &L->Af); mat_free_host(h, &L->W); mat_free_host(h, &L->AfP);
    apart_free(&L->Pn);
    apart_free(&L->Pf);
  }
  amgd_vc_plan_free_host(&h->plan);
  amgd_kry_ws_free_host(&h->kry);
  amgd_kry_nws_free_host(&h->kryn);
  free(h->lv);
  free(h);
  *hp = NULL;
}
