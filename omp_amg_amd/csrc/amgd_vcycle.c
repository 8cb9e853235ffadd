/*
 * amgd_vcycle.c -- the AMG V-cycle on the device-resident hierarchy (host driver, C).
 *
 * Applies the reference's amg_exec (amg.c:114-169) to the hierarchy as this library stores
 * it (CSR, ascending columns): restriction b_{l+1} += W' b_l[F] down the levels, the 1 x 1
 * bottom solve, then per level xf = W xc, bf = b[F] - AfP xc and m Chebyshev steps on Af
 * with the scaled diagonal D (DESIGN.md "Solve" has the contract).
 *
 * Layout: the reference's level-ordered vector (lvl_offset, amg.c:117).  Position
 * off[l] + k holds the k-th F point of level l and the bottom point comes last, so level
 * l's whole vector is the tail [off[l], N) of one flat array and its coarse part the tail
 * [off[l+1], N): no kernel gathers through a C/F mask, every level works on slices.  The
 * plan keeps pos_0 (level-0 row -> position), per level the columns of W and AfP renumbered
 * to positions relative to off[l+1] (values, row offsets and entry order are the
 * hierarchy's), W' by the stable transpose (ascending F row per column, rows in position
 * order), and the flat work vectors.  It is built on the first solve of a hierarchy and
 * freed with it.
 *
 * Two paths, bit-identical: composed (amgd_spmv and the vector kernels -- only kernels the
 * setup already had, plus one elementwise update) and fused (amgd_solve.hip), chosen per
 * product by row shape: the short-row kernels below a mean row of 16, the cooperative
 * long-row kernels (off by default: they measured slower than the composed form) above,
 * composed for a matrix with an outlier row; the deepest levels in one workgroup.  Compiled with -ffp-contract=off: the Chebyshev scalars round like
 * the reference's.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "amgd.h"
#include "amgd_drv.h"
#include "omp_amg_amd.h"

#define API __attribute__((visibility("default")))

/* rows longer than this leave the thread-per-row kernels to the composed path */
#define VC_ROW_MAX 4096u
/* mean row length from which a product is a long-row shape (amgd_sparse.hip WAVE_ROWS_MIN_MEAN) */
#define VC_THR_MEAN 16u
#define VC_COOP_DEFAULT 0
/* by default the tail takes only levels whose matrix entries, all passes together, number at
   most this many: one workgroup walks them alone (DESIGN.md "Solve", the measured table) */
#define VC_TAIL_WORK 16384ull

enum { VC_COMP = 0, VC_THR = 1, VC_COOP = 2 };
typedef struct {
  uint32_t nf, nc, off, steps;      /* F rows, coarse positions (= N - off - nf), steps = m - 1 */
  double *beta, *gamma;             /* per Chebyshev update (host) */
  dcsr W, AfP;                      /* the hierarchy's ro / a, own col (positions) */
  dcsr *Wt;                         /* (W in positions)' */
  const dcsr *Af;
  const double *D;
  int sh_r, sh_p, sh_c;             /* form of restriction / prolongation / Chebyshev: VC_COMP .. */
} vc_lev;

struct amgd_vc_plan {
  uint32_t nl, N, tail_first, tail_rows;   /* levels, positions; tail: levels tail_first .. nl-2 */
  vc_lev *lv;                              /* nl - 1 */
  uint32_t **hpos;                         /* build only */
  uint32_t *pos0;
  double *b, *x, *c0, *c1, *r, *ones, *dbotv;
  double dbot;
  amgd_vc_tlev *tail;                      /* device */
  uint64_t bytes, tail_cap;
  int tail_set;                            /* the tail was laid out for (tail_rows, tail_cap) */
};

static int g_fused = -1, g_tail = -1, g_coop = -1;
void amgd_vc_set_fused(int on) { g_fused = on; }
void amgd_vc_set_coop(int on) { g_coop = on; }
void amgd_vc_set_tail(int rows) { g_tail = rows > AMGD_VC_TAIL_ROWS ? AMGD_VC_TAIL_ROWS : rows; }
/* the environment's switches, read once: AMGD_VC_FUSED, AMGD_VC_COOP (the cooperative form for
   long-row shapes; default: DESIGN.md "Solve", the measured table), AMGD_VC_TAIL,
   AMGD_VC_TAIL_WORK */
static struct { int read, fused, coop; uint32_t tail; uint64_t work; } g_env;
static void env_read(void) {
  if (g_env.read) return;
  const char *e = getenv("AMGD_VC_FUSED");
  g_env.fused = !(e && *e == '0');
  e = getenv("AMGD_VC_COOP");
  g_env.coop = e && *e ? *e != '0' : VC_COOP_DEFAULT;
  e = getenv("AMGD_VC_TAIL");
  g_env.tail = e && *e == '0' ? 0 : AMGD_VC_TAIL_ROWS;
  e = getenv("AMGD_VC_TAIL_WORK");
  g_env.work = e && *e ? strtoull(e, NULL, 10) : VC_TAIL_WORK;
  g_env.read = 1;
}
static int coop_on(void) { env_read(); return g_coop < 0 ? g_env.coop : g_coop; }
static int fused_on(void) { env_read(); return g_fused < 0 ? g_env.fused : g_fused; }
static uint32_t tail_rows(void) { env_read(); return g_tail < 0 ? g_env.tail : (uint32_t)g_tail; }
/* an explicit limit (amgd_vc_set_tail) is by rows alone */
static uint64_t tail_work(void) { env_read(); return g_tail >= 0 ? ~0ull : g_env.work; }

/* the scalar recurrences of amg_exec in the reference's operation order (amg.c:148-149, :158) */
static void cheb_scalars(double rho, uint32_t m, double *beta_out, double *gamma_out) {
  if (m < 2) return;
  double alpha, beta, gamma;
  alpha = rho / 2, alpha *= alpha;
  gamma = 2 * alpha / (1 - 2 * alpha), beta = 1 + gamma;
  beta_out[0] = beta;
  gamma_out[0] = gamma;
  for (uint32_t ci = 3; ci <= m; ++ci) {
    gamma = alpha * beta, gamma = gamma / (1 - gamma), beta = 1 + gamma;
    beta_out[ci - 2] = beta;
    gamma_out[ci - 2] = gamma;
  }
}

/* the fused form of a matrix's products: thread per row for a short mean row, cooperative
   from WAVE_ROWS_MIN_MEAN on, composed when a row is an outlier */
static int mat_shape(const dcsr *M) {
  if (!M->rn || !M->nnz) return VC_THR;
  amgd_rowmax_pin(M);
  const uint32_t mx = amgd_max_row_len(M);
  amgd_rowmax_unpin(M);
  if (mx > VC_ROW_MAX) return VC_COMP;
  return M->nnz >= (uint64_t)VC_THR_MEAN * M->rn ? VC_COOP : VC_THR;
}
static void lev_shapes(vc_lev *L) {
  L->sh_r = mat_shape(L->Wt);
  const int a = mat_shape(&L->W), b = mat_shape(&L->AfP);   /* one kernel walks both */
  L->sh_p = a == VC_COMP || b == VC_COMP ? VC_COMP : a == VC_COOP || b == VC_COOP ? VC_COOP : VC_THR;
  L->sh_c = L->steps ? mat_shape(L->Af) : VC_THR;
}
/* the form a product takes now */
static int form(int shape, int fused) {
  if (!fused || shape == VC_COMP || (shape == VC_COOP && !coop_on())) return VC_COMP;
  return shape;
}
/* launches of the cycles so far, NOMINAL: tallied per product from the form it took (one per
   fused kernel, one per amgd_spmv / vector kernel of a composed product), not counted at the
   launch sites -- amgd_spmv's outlier-row path launches more than one kernel */
static uint64_t g_launches;
uint64_t amgd_vc_launches(void) { return g_launches; }
static void form_hit(int f) {
  amgd_route_hit(f == VC_THR ? AMGD_R_VC_THR : f == VC_COOP ? AMGD_R_VC_WAVE : AMGD_R_VC_COMP);
}

/* restriction of one level: bC += W' bF */
static void vc_restrict(const vc_lev *L, double *bF, double *bC, int fused) {
  const int f = form(L->sh_r, fused);
  form_hit(f);
  g_launches++;
  if (f == VC_THR) amgd_vc_restrict_thr(L->Wt, bF, bC);
  else if (f == VC_COOP) amgd_vc_restrict_coop(L->Wt, bF, bC);
  else amgd_spmv(L->Wt, bF, bC, 1., bC, 1., NULL);
}
/* up-sweep of one level (amg.c:139-166); returns the buffer holding the last c */
static double *vc_up(const vc_lev *L, const double *xc, double *xf, double *bf, double *c0, double *c1,
                     double *r, int fused) {
  const uint32_t nf = L->nf;
  const int fp = form(L->sh_p, fused), fc = form(L->sh_c, fused);
  form_hit(fp);
  g_launches += fp != VC_COMP ? 1 : L->steps == 0 ? 4 : 3;
  if (fp == VC_THR) {
    amgd_vc_prolong_thr(&L->W, &L->AfP, L->D, xc, xf, bf, c0, L->steps == 0);
  } else if (fp == VC_COOP) {
    amgd_vc_prolong_coop(&L->W, &L->AfP, L->D, xc, xf, bf, c0, L->steps == 0);
  } else {
    amgd_spmv(&L->W, xc, xf, 0., NULL, 1., NULL);          /* x_l = W x_{l+1} */
    amgd_spmv(&L->AfP, xc, bf, 1., bf, -1., NULL);         /* b_l -= AfP x_{l+1} */
    amgd_vop(c0, L->D, bf, nf, AMGD_V_MUL);                /* c_1 = Dff b_l */
    if (L->steps == 0) amgd_vop(xf, xf, c0, nf, AMGD_V_ADD);
  }
  double *c = c0, *cn = c1;
  for (uint32_t k = 0; k < L->steps; k++) {
    const int last = k + 1 == L->steps;
    form_hit(fc);
    g_launches += fc != VC_COMP ? 1 : last ? 3 : 2;
    if (fc == VC_THR) {
      amgd_vc_cheb_thr(L->Af, L->D, bf, c, cn, L->beta[k], L->gamma[k], k > 0, last ? xf : NULL);
    } else if (fc == VC_COOP) {
      amgd_vc_cheb_coop(L->Af, L->D, bf, c, cn, L->beta[k], L->gamma[k], k > 0, last ? xf : NULL);
    } else {
      amgd_spmv(L->Af, c, r, 1., bf, -1., NULL);           /* r_i = b_l - Aff c_i */
      amgd_vc_cheb_update(cn, c, L->D, r, L->beta[k], L->gamma[k], k > 0, nf);
      if (last) amgd_vop(xf, xf, cn, nf, AMGD_V_ADD);
    }
    double *t = c; c = cn; cn = t;
  }
  return c;
}

static void tlev_fill(amgd_vc_tlev *T, const vc_lev *L) {
  memset(T, 0, sizeof *T);
  T->wt_ro = L->Wt->ro; T->wt_col = L->Wt->col; T->wt_a = L->Wt->a;
  T->w_ro = L->W.ro; T->w_col = L->W.col; T->w_a = L->W.a;
  T->p_ro = L->AfP.ro; T->p_col = L->AfP.col; T->p_a = L->AfP.a;
  T->af_ro = L->Af->ro; T->af_col = L->Af->col; T->af_a = L->Af->a;
  T->D = L->D;
  T->nf = L->nf; T->nc = L->nc; T->off = L->off; T->steps = L->steps;
  for (uint32_t k = 0; k < L->steps && k < AMGD_VC_MAXSTEPS; k++) { T->beta[k] = L->beta[k]; T->gamma[k] = L->gamma[k]; }
}

/* ------------------------------------------------------------------------ */
/* plan                                                                      */
/* ------------------------------------------------------------------------ */
void amgd_vc_plan_free_host(struct amgd_vc_plan **pp) {
  struct amgd_vc_plan *p = *pp;
  if (!p) return;
  if (p->lv)
    for (uint32_t l = 0; l + 1 < p->nl; l++) { free(p->lv[l].beta); free(p->lv[l].gamma); free(p->lv[l].Wt); }
  if (p->hpos) { for (uint32_t l = 0; l < p->nl; l++) free(p->hpos[l]); free(p->hpos); }
  free(p->lv);
  free(p);
  *pp = NULL;
}
void amgd_vc_plan_free(struct amgd_vc_plan **pp) {
  struct amgd_vc_plan *p = *pp;
  if (!p) return;
  for (uint32_t l = 0; l + 1 < p->nl; l++) {
    vc_lev *L = &p->lv[l];
    if (L->W.col) amgd_free(L->W.col);
    if (L->AfP.col) amgd_free(L->AfP.col);
    if (L->Wt) { amgd_free(L->Wt->ro); amgd_free(L->Wt->col); amgd_free(L->Wt->a); }
  }
  if (p->pos0) amgd_free(p->pos0);
  if (p->b) amgd_free(p->b);
  if (p->x) amgd_free(p->x);
  if (p->c0) amgd_free(p->c0);
  if (p->c1) amgd_free(p->c1);
  if (p->r) amgd_free(p->r);
  if (p->ones) amgd_free(p->ones);
  if (p->dbotv) amgd_free(p->dbotv);
  if (p->tail) amgd_free(p->tail);
  amgd_vc_plan_free_host(pp);
}

typedef struct { const amgd_hier *h; struct amgd_vc_plan *p; } plan_args;
/* columns of M (level l's W or AfP) as positions relative to off[l+1] */
static uint32_t *remap(const dcsr *M, const uint32_t *dpos, uint32_t off_next) {
  uint32_t *col = (uint32_t *)amgd_alloc(M->nnz * 4 + 4);
  amgd_vc_remap_cols(M->col, M->nnz, dpos, off_next, col);
  return col;
}
static int plan_body(void *arg) {
  plan_args *pa = (plan_args *)arg;
  const amgd_hier *h = pa->h;
  const uint32_t nl = h->nlevels;
  struct amgd_vc_plan *p = (struct amgd_vc_plan *)calloc(1, sizeof *p);
  pa->p = p;
  p->nl = nl;
  p->lv = (vc_lev *)calloc(nl, sizeof(vc_lev));
  p->hpos = (uint32_t **)calloc(nl, sizeof(uint32_t *));
  /* sizes, offsets */
  uint32_t off = 0, maxnf = 1;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const amgd_level *H = &h->lv[l];
    vc_lev *L = &p->lv[l];
    L->nf = H->Af.d->rn;
    L->off = off;
    off += L->nf;
    if (L->nf > maxnf) maxnf = L->nf;
    if (H->A.d->rn != L->nf + h->lv[l + 1].A.d->rn) { amgd_set_error("amgd_solve: level sizes do not add up"); return -1; }
  }
  if (h->lv[nl - 1].A.d->rn != 1 || off + 1 != h->n0) { amgd_set_error("amgd_solve: the hierarchy does not end in a 1 x 1 level"); return -1; }
  const uint32_t N = p->N = off + 1;
  for (uint32_t l = 0; l + 1 < nl; l++) p->lv[l].nc = N - p->lv[l].off - p->lv[l].nf;
  /* positions, bottom up: pos_l[F] = off[l] + 0..nf-1, pos_l[C] = pos_{l+1} */
  p->hpos[nl - 1] = (uint32_t *)malloc(4);
  p->hpos[nl - 1][0] = N - 1;
  for (uint32_t l = nl - 1; l-- > 0;) {
    const uint32_t n = h->lv[l].A.d->rn;
    uint8_t *vc = (uint8_t *)malloc((size_t)n + 1);
    amgd_d2h(vc, h->lv[l].vc, n);
    uint32_t *pos = p->hpos[l] = (uint32_t *)malloc((size_t)n * 4 + 4);
    uint32_t kf = 0, kc = 0;
    const uint32_t ncn = h->lv[l + 1].A.d->rn;
    int ok = 1;
    for (uint32_t i = 0; i < n && ok; i++) {
      if (vc[i]) { if (kc < ncn) pos[i] = p->hpos[l + 1][kc++]; else ok = 0; }
      else { if (kf < p->lv[l].nf) pos[i] = p->lv[l].off + kf++; else ok = 0; }
    }
    free(vc);
    if (!ok || kc != ncn || kf != p->lv[l].nf) { amgd_set_error("amgd_solve: a C/F mask does not match its level's sizes"); return -1; }
  }
  /* per level: renumbered columns, W', scalars, shapes */
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const amgd_level *H = &h->lv[l];
    vc_lev *L = &p->lv[l];
    const uint32_t nn = h->lv[l + 1].A.d->rn, off_next = L->off + L->nf;
    uint32_t *dpos = (uint32_t *)amgd_alloc((size_t)nn * 4 + 4);
    amgd_h2d(dpos, p->hpos[l + 1], (size_t)nn * 4);
    L->W = *H->W.d;
    L->W.col = NULL;
    L->AfP = *H->AfP.d;
    L->AfP.col = NULL;
    L->W.col = remap(H->W.d, dpos, off_next);
    L->AfP.col = remap(H->AfP.d, dpos, off_next);
    amgd_free(dpos);
    L->Wt = amgd_transpose(&L->W, NULL);
    L->Af = H->Af.d;
    L->D = H->D;
    const uint32_t m = H->m >= 1 ? (uint32_t)H->m : 1;
    L->steps = m - 1;
    L->beta = (double *)calloc(m, 8);
    L->gamma = (double *)calloc(m, 8);
    cheb_scalars(H->rho, m, L->beta, L->gamma);
    lev_shapes(L);
  }
  p->pos0 = (uint32_t *)amgd_alloc((size_t)N * 4 + 4);
  amgd_h2d(p->pos0, p->hpos[0], (size_t)N * 4);
  for (uint32_t l = 0; l < nl; l++) { free(p->hpos[l]); p->hpos[l] = NULL; }
  free(p->hpos);
  p->hpos = NULL;
  p->b = dalloc(N); p->x = dalloc(N); p->ones = dones(N);
  p->c0 = dalloc(maxnf); p->c1 = dalloc(maxnf); p->r = dalloc(maxnf);
  /* x = d*b with d = 0 on a null space, else 1./a (amg_setup.c:441-450) */
  double a0 = 0;
  if (h->lv[nl - 1].A.d->nnz) amgd_d2h(&a0, h->lv[nl - 1].A.d->a, 8);
  p->dbot = h->nullspace != 0 ? 0. : 1. / a0;
  p->dbotv = dalloc(1);
  amgd_h2d(p->dbotv, &p->dbot, 8);
  /* the tail: the levels from the first whose slice [off[l], N) fits one workgroup */
  p->tail_first = nl - 1;
  p->tail_rows = 0;
  /* algorithmic bytes of one cycle: 12 B per entry of each matrix pass, 8 B per vector
     element read or written; in and out of the level-ordered layout: 4 N elements */
  p->bytes = 4ull * 8 * N;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const vc_lev *L = &p->lv[l];
    const uint64_t nf = L->nf, nc = L->nc, st = L->steps;
    p->bytes += 12 * (L->Wt->nnz + L->W.nnz + L->AfP.nnz + st * L->Af->nnz);
    p->bytes += 8 * (nf + 2 * nc);                         /* restriction: bF, bC in and out */
    p->bytes += 8 * (nc + 5 * nf);                         /* xc; xf, bf in and out, D, c */
    p->bytes += 8 * st * 4 * nf + (st > 1 ? 8 * (st - 1) * nf : 0) + (st ? 16 * nf : 0);
  }
  return 0;
}
/* (re)build the tail's descriptors for the row limit in force */
static void plan_tail(struct amgd_vc_plan *p) {
  const uint32_t rows = tail_rows();
  const uint64_t cap = tail_work();
  if (p->tail_set && rows == p->tail_rows && cap == p->tail_cap) return;
  if (p->tail) { amgd_free(p->tail); p->tail = NULL; }
  p->tail_set = 0;
  p->tail_first = p->nl - 1;
  uint32_t first = p->nl - 1;
  uint64_t work = 0;
  for (uint32_t l = p->nl - 1; l-- > 0;) {
    const vc_lev *L = &p->lv[l];
    work += L->Wt->nnz + L->W.nnz + L->AfP.nnz + (uint64_t)L->steps * L->Af->nnz;
    if (p->N - L->off > rows || work > cap) break;
    first = l;
  }
  for (uint32_t l = first; l + 1 < p->nl; l++)
    if (p->lv[l].steps > AMGD_VC_MAXSTEPS) first = p->nl - 1;
  const uint32_t nt = p->nl - 1 - first;
  if (nt) {
    /* the device block first: out of HBM unwinds from here with no host block held */
    amgd_vc_tlev *dT = (amgd_vc_tlev *)amgd_alloc(nt * sizeof *dT);
    amgd_vc_tlev *T = (amgd_vc_tlev *)calloc(nt, sizeof *T);
    for (uint32_t q = 0; q < nt; q++) tlev_fill(&T[q], &p->lv[first + q]);
    amgd_h2d(dT, T, nt * sizeof *T);
    free(T);
    p->tail = dT;
  }
  p->tail_first = first;
  p->tail_rows = rows;
  p->tail_cap = cap;
  p->tail_set = 1;
}

/* ------------------------------------------------------------------------ */
/* the cycle                                                                 */
/* ------------------------------------------------------------------------ */
static uint64_t g_cycles, g_bytes_last;
/* the cycles' own event timer (amgd_rt.hip): a setup's timer reset does not touch it */
void amgd_timers_enable(int on);
void amgd_vc_timer_begin(void);
void amgd_vc_timer_end(void);
double amgd_vc_timer_ms(void);
void amgd_vc_timer_zero(void);
#define VC_DRAIN 256                     /* cycles between two reads of the pending events */

static void cycle(struct amgd_vc_plan *p) {
  const int fused = fused_on();
  const uint32_t nl = p->nl, N = p->N;
  uint32_t tf = p->tail ? p->tail_first : nl - 1;
  for (uint32_t l = 0; l < tf; l++) {
    const vc_lev *L = &p->lv[l];
    vc_restrict(L, p->b + L->off, p->b + L->off + L->nf, fused);
  }
  if (tf < nl - 1) {
    amgd_route_hit(AMGD_R_VC_TAIL);
    g_launches++;
    amgd_vc_tail(p->tail, (int)(nl - 1 - tf), p->b, p->x, p->c0, p->c1, N, p->dbot, 0);
  } else {
    g_launches++;
    amgd_vop(p->x + N - 1, p->dbotv, p->b + N - 1, 1, AMGD_V_MUL);       /* x = d*b (amg.c:130) */
  }
  for (uint32_t l = tf; l-- > 0;) {
    const vc_lev *L = &p->lv[l];
    vc_up(L, p->x + L->off + L->nf, p->x + L->off, p->b + L->off, p->c0, p->c1, p->r, fused);
  }
}

typedef struct { amgd_hier *h; } tail_args;
static int tail_body(void *arg) { plan_tail(((tail_args *)arg)->h->plan); return 0; }
/* sum(x) left to right in the level-ordered layout, through the exact-dot path */
typedef struct { const struct amgd_vc_plan *p; double sum; } sum_args;
static int sum_body(void *arg) {
  sum_args *sa = (sum_args *)arg;
  sa->sum = amgd_dot(sa->p->x, sa->p->ones, sa->p->N);
  return 0;
}

API int amgd_solve_device(amgd_hier *h, double *dx, const double *db, int flags) {
  if (!h || h->nlevels == 0 || h->n0 == 0 || !dx || !db) return -1;
  if (h->part) return -3;
  if (!h->plan) {
    plan_args a = {h, NULL};
    const int rc = amgd_try(plan_body, &a);
    if (rc != 0) {
      if (rc == -2) amgd_vc_plan_free_host(&a.p);     /* device blocks: released by the unwind */
      else amgd_vc_plan_free(&a.p);
      return rc == -2 ? -2 : -1;
    }
    h->plan = a.p;
  }
  struct amgd_vc_plan *p = h->plan;
  tail_args ta = {h};
  if (amgd_try(tail_body, &ta) != 0) { p->tail = NULL; p->tail_set = 0; p->tail_first = p->nl - 1; return -2; }
  /* the setup's event timers (the long-row SpMV's slots) stay off inside a cycle: only a
     setup's statistics read them, so a solve must not queue events on them */
  amgd_vc_timer_begin();
  amgd_timers_enable(0);
  amgd_vc_scatter(p->b, db, p->pos0, p->N);
  cycle(p);
  amgd_timers_enable(1);
  amgd_vc_timer_end();
  g_launches += 2;                                     /* into and out of the level-ordered layout */
  g_cycles++;
  g_bytes_last = p->bytes;
  if (g_cycles % VC_DRAIN == 0) (void)amgd_vc_timer_ms();   /* hand the timing events back */
  double avg = 0;
  if (flags & 1) {
    /* x -= (1/n) sum(x), the sum left to right in the level-ordered layout (amg.c:181-184) */
    sum_args sa = {p, 0.};
    const int ex = amgd_get_exact();
    amgd_set_exact(1);
    const int rc = amgd_try(sum_body, &sa);
    amgd_set_exact(ex);
    if (rc != 0) return -2;
    const double tni = 1. / (double)p->N;
    avg = tni * sa.sum;
  }
  amgd_vc_gather(dx, p->x, p->pos0, p->N, flags & 1, avg);
  return 0;
}

API void amgd_solve_stats(uint64_t *cycles, double *ms, uint64_t *bytes) {
  if (cycles) *cycles = g_cycles;
  if (ms) *ms = amgd_vc_timer_ms();
  if (bytes) *bytes = g_bytes_last;
}
void amgd_vc_stats_reset(void) {
  amgd_vc_timer_zero();
  g_cycles = 0;
}

/* ------------------------------------------------------------------------ */
/* test hooks' cores (amgd_testapi.c): one level on given device operands    */
/* ------------------------------------------------------------------------ */
/* mode 0 composed, 1 fused, 2 the tail kernel (up-sweep only; nf + nc <= 1024, else -1).
   x and b: nf + nc doubles each (xc behind xf, bf first); c_out: nf */
int amgd_vc_level_run(const dcsr *Af, const dcsr *W, const dcsr *AfP, const double *D, uint32_t m, double rho,
                      double *x, double *b, double *c_out, int mode) {
  vc_lev L;
  memset(&L, 0, sizeof L);
  L.nf = W->rn; L.nc = W->cn; L.off = 0;
  L.steps = m ? m - 1 : 0;
  L.beta = (double *)calloc(m + 1, 8);
  L.gamma = (double *)calloc(m + 1, 8);
  cheb_scalars(rho, m, L.beta, L.gamma);
  L.W = *W; L.AfP = *AfP; L.Af = Af; L.D = D;
  dcsr none = {0, 0, 0, NULL, NULL, NULL};
  L.Wt = &none;
  lev_shapes(&L);
  double *c0 = dalloc(L.nf), *c1 = dalloc(L.nf), *r = dalloc(L.nf);
  const double *c = NULL;
  int rc = 0;
  if (mode == 2) {
    if (L.nf + L.nc > AMGD_VC_TAIL_ROWS || L.steps > AMGD_VC_MAXSTEPS) rc = -1;
    else {
      amgd_vc_tlev T;
      tlev_fill(&T, &L);
      amgd_vc_tlev *dT = (amgd_vc_tlev *)amgd_alloc(sizeof T);
      amgd_h2d(dT, &T, sizeof T);
      amgd_route_hit(AMGD_R_VC_TAIL);
      amgd_vc_tail(dT, 1, b, x, c0, c1, L.nf + L.nc, 0., 1);
      amgd_sync();
      amgd_free(dT);
      c = L.steps % 2 ? c1 : c0;
    }
  } else {
    c = vc_up(&L, x + L.nf, x, b, c0, c1, r, mode);
  }
  if (c) amgd_d2d(c_out, c, (size_t)L.nf * 8);
  amgd_sync();
  amgd_free(c0); amgd_free(c1); amgd_free(r);
  free(L.beta); free(L.gamma);
  return rc;
}
/* bC += W' bF with W' = amgd_transpose(W) */
void amgd_vc_restrict_run(const dcsr *W, double *bF, double *bC, int fused) {
  vc_lev L;
  memset(&L, 0, sizeof L);
  L.Wt = amgd_transpose(W, NULL);
  L.sh_r = mat_shape(L.Wt);
  vc_restrict(&L, bF, bC, fused);
  amgd_sync();
  dcsr_free(&L.Wt);
}
