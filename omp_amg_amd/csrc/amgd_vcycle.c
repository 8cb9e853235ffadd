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
 *
 * A row-partitioned hierarchy (amgd_part.h) is solved by the same code on each rank's rows
 * (second half of the plan and of the cycle below): the rank's blocks of W, AfP, Af and of W'
 * per distributed level, a halo exchange (or an allgatherv of the F segment) before each
 * product that reads another rank's entries, and the coarse levels replicated on every rank
 * through the one-GPU path -- bit-identical to the one-GPU cycle on the gathered hierarchy.
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

/* The partitioned cycle (DESIGN.md "Solve", the partitioned part).  A rank owns, per level,
   the positions off[l] + [Pf_l.split[me], Pf_l.split[me+1]) and runs the row kernels on its
   rows; the levels from lt on are replicated: whole matrices on every rank, the one-GPU code.
   One halo exchange: the entries of a vector that this rank's rows reference and another
   rank owns, fetched with pack -> alltoallv -> unpack. */
typedef struct {
  uint64_t nsend, nrecv;            /* entries this rank packs / receives */
  uint32_t *sidx, *ridx;            /* device: entries to pack, peer by peer / places of the received */
  uint64_t *soff, *roff;            /* host, np + 1 each: byte offsets by peer */
  uint64_t total;                   /* entries all ranks move: 0 = every rank skips the exchange */
} vc_halo;
typedef struct {
  vc_lev L;                         /* own rows of W, AfP (columns: positions) and Af; Wt: own C rows */
  uint32_t f0;                      /* first own F point */
  pmat *Wt;                         /* pm_transpose(W): columns are F indices, ascending F row per column */
  uint32_t *cmap;                   /* device: own C row -> position */
  vc_halo hb, hx, hc;               /* bF for W'; xc for W and AfP; c for Af */
  uint64_t *agoff;                  /* host, np + 1: the F segment's byte offsets by rank */
} vc_plev;

struct amgd_vc_plan {
  uint32_t nl, N, tail_first, tail_rows;   /* levels, positions; tail: levels tail_first .. nl-2 */
  vc_lev *lv;                              /* nl - 1 (partitioned: nf / nc / off of every level, the
                                              matrices of the replicated ones) */
  int part, np, me;                        /* partitioned: ranks, this rank */
  uint32_t lt, r0, r1;                     /* first replicated level (one GPU: 0); own level-0 rows */
  uint64_t repl;                           /* the replication limit lt was chosen for */
  vc_plev *pl;                             /* levels 0 .. lt-1 */
  vc_halo h0;                              /* a whole level-0 vector for the own rows of A (amgd_krylov.c) */
  dcsr **gath;                             /* 3 per level: gathered Af, W, AfP of the replicated levels */
  double *sbuf, *rbuf;                     /* halo send / receive buffers */
  uint64_t *downoff, *xoff, *dxoff;        /* host: allgatherv offsets of b's replicated slice, x, dx */
  uint64_t down_bytes, x_bytes;            /* bytes all ranks send in those */
  uint32_t **hpos;                         /* build only */
  uint32_t *pos0;
  double *b, *x, *c0, *c1, *r, *ones, *dbotv;
  double dbot;
  /* several right-hand sides: the interleaved work vectors of a group of nk columns (N * nk
     doubles each; 0: not allocated yet), grown to the largest group size used so far */
  uint32_t nk;
  double *nb, *nx, *nc0, *nc1;
  uint64_t mbytes;                         /* the matrix part of bytes */
  amgd_vc_tlev *tail;                      /* device */
  uint64_t bytes, tail_cap;
  int tail_set;                            /* the tail was laid out for (tail_rows, tail_cap) */
};

/* vc_coop: the cooperative form for long-row shapes (default: DESIGN.md "Solve", the measured
   table).  vc_repl: levels whose slice [off[l], N) has at most that many positions are
   replicated (DESIGN.md "Solve": reasoned from the levels' byte counts, not measured).
   vc_tail_work: by default the tail takes only levels whose matrix entries, all passes
   together, number at most that many: one workgroup walks them alone */
static int coop_on(void) { return amgd_knob(AMGD_K_VC_COOP) != 0; }
static int fused_on(void) { return amgd_knob(AMGD_K_VC_FUSED) != 0; }
static int halo_on(void) { return amgd_knob(AMGD_K_VC_HALO) != 0; }
static uint64_t repl_rows(void) { return (uint64_t)amgd_knob(AMGD_K_VC_REPL); }
/* the variable is on / off; an override is a row limit, and then the only limit */
static uint32_t tail_rows(void) {
  const int64_t t = amgd_knob(AMGD_K_VC_TAIL);
  if (amgd_knob_source(AMGD_K_VC_TAIL) != 2) return t ? AMGD_VC_TAIL_ROWS : 0;
  return (uint32_t)(t > AMGD_VC_TAIL_ROWS ? AMGD_VC_TAIL_ROWS : t < 0 ? 0 : t);
}
static uint64_t tail_work(void) {
  return amgd_knob_source(AMGD_K_VC_TAIL) == 2 ? ~0ull : (uint64_t)amgd_knob(AMGD_K_VC_TAIL_WORK);
}

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
/* tests: a lower outlier limit makes small fixtures take the outlier-row paths (0: VC_ROW_MAX).
   Read when a plan is built, and by the single-vector plan as well as the multi-RHS cycle: a
   process-wide setting that every plan built while it is set carries, so a test puts it back
   before anything else builds one */
static uint32_t row_max(void) {
  const int64_t n = amgd_knob(AMGD_K_VC_ROW_MAX);
  return n > 0 ? (uint32_t)n : VC_ROW_MAX;
}
static int mat_shape(const dcsr *M) {
  if (!M->rn || !M->nnz) return VC_THR;
  amgd_rowmax_pin(M);
  const uint32_t mx = amgd_max_row_len(M);
  amgd_rowmax_unpin(M);
  if (mx > row_max()) return VC_COMP;
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

/* b += Wt bF in form f; map NULL: b is the coarse slice, else row c adds into b[map[c]] and the
   composed form goes through r (Wt->rn doubles) */
static void restrict_as(int f, const dcsr *Wt, const double *bF, double *b, const uint32_t *map, double *r) {
  if (f != VC_COMP) amgd_vc_restrict(f == VC_COOP, 1, Wt, bF, b, map);
  else if (!map) amgd_spmv(Wt, bF, b, 1., b, 1., NULL);
  else {
    amgd_spmv(Wt, bF, r, 0., NULL, 1., NULL);
    amgd_vc_add_map(b, map, r, Wt->rn);
  }
}
/* restriction of one level: bC += W' bF */
static void vc_restrict(const vc_lev *L, double *bF, double *bC, int fused) {
  const int f = form(L->sh_r, fused);
  form_hit(f);
  g_launches++;
  restrict_as(f, L->Wt, bF, bC, NULL, NULL);
}
/* up-sweep of one level (amg.c:139-166); returns the buffer holding the last c.  A rank's row
   block (partitioned cycle) passes X: L holds its rows, xf / bf / L->D start at its first row,
   c0 / c1 / r are the whole buffers with its rows at f0, and every Af product is preceded by
   the exchange that brings in the entries of c its rows reference */
typedef struct { uint32_t f0; void (*c_exchange)(void *ctx, double *c); void *ctx; } vc_rows;
static double *vc_up(const vc_lev *L, const double *xc, double *xf, double *bf, double *c0, double *c1,
                     double *r, int fused, const vc_rows *X) {
  const uint32_t nf = L->nf, f0 = X ? X->f0 : 0;
  if (X && !nf) {                                          /* a rank with no row here: the exchanges only */
    double *c = c0, *cn = c1;
    for (uint32_t k = 0; k < L->steps; k++) { X->c_exchange(X->ctx, c); double *t = c; c = cn; cn = t; }
    return c;
  }
  const int fp = form(L->sh_p, fused), fc = form(L->sh_c, fused);
  form_hit(fp);
  g_launches += fp != VC_COMP ? 1 : L->steps == 0 ? 4 : 3;
  if (fp != VC_COMP) {
    amgd_vc_prolong(fp == VC_COOP, 1, &L->W, &L->AfP, L->D, xc, xf, bf, c0 + f0, L->steps == 0);
  } else {
    amgd_spmv(&L->W, xc, xf, 0., NULL, 1., NULL);          /* x_l = W x_{l+1} */
    amgd_spmv(&L->AfP, xc, bf, 1., bf, -1., NULL);         /* b_l -= AfP x_{l+1} */
    amgd_vop(c0 + f0, L->D, bf, nf, AMGD_V_MUL);           /* c_1 = Dff b_l */
    if (L->steps == 0) amgd_vop(xf, xf, c0 + f0, nf, AMGD_V_ADD);
  }
  double *c = c0, *cn = c1;
  for (uint32_t k = 0; k < L->steps; k++) {
    const int last = k + 1 == L->steps;
    if (X) X->c_exchange(X->ctx, c);
    form_hit(fc);
    g_launches += fc != VC_COMP ? 1 : last ? 3 : 2;
    if (fc != VC_COMP) {
      amgd_vc_cheb(fc == VC_COOP, 1, L->Af, L->D, bf, c, c + f0, cn + f0, L->beta[k], L->gamma[k], k > 0,
                   last ? xf : NULL);
    } else {
      amgd_spmv(L->Af, c, r + f0, 1., bf, -1., NULL);      /* r_i = b_l - Aff c_i */
      amgd_vc_cheb_update(cn + f0, c + f0, L->D, r + f0, L->beta[k], L->gamma[k], k > 0, nf);
      if (last) amgd_vop(xf, xf, cn + f0, nf, AMGD_V_ADD);
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
static void halo_free_host(vc_halo *H) { free(H->soff); free(H->roff); }
static void halo_free(vc_halo *H) {
  if (H->sidx) amgd_free(H->sidx);
  if (H->ridx) amgd_free(H->ridx);
}
void amgd_vc_plan_free_host(struct amgd_vc_plan **pp) {
  struct amgd_vc_plan *p = *pp;
  if (!p) return;
  if (p->lv)
    for (uint32_t l = 0; l + 1 < p->nl; l++) {
      free(p->lv[l].beta); free(p->lv[l].gamma);
      if (!p->part) free(p->lv[l].Wt);
    }
  if (p->pl)
    for (uint32_t l = 0; l < p->lt; l++) {
      vc_plev *P = &p->pl[l];
      if (P->Wt) { free(P->Wt->m); free(P->Wt); }
      free(P->L.beta); free(P->L.gamma);
      halo_free_host(&P->hb); halo_free_host(&P->hx); halo_free_host(&P->hc);
      free(P->agoff);
    }
  halo_free_host(&p->h0);
  if (p->gath) { for (uint32_t k = 0; k < 3 * p->nl; k++) free(p->gath[k]); free(p->gath); }
  if (p->part && p->lv) for (uint32_t l = p->lt; l + 1 < p->nl; l++) free(p->lv[l].Wt);
  if (p->hpos) { for (uint32_t l = 0; l < p->nl; l++) free(p->hpos[l]); free(p->hpos); }
  free(p->downoff); free(p->xoff); free(p->dxoff);
  free(p->pl);
  free(p->lv);
  free(p);
  *pp = NULL;
}
void amgd_vc_plan_free(struct amgd_vc_plan **pp) {
  struct amgd_vc_plan *p = *pp;
  if (!p) return;
  for (uint32_t l = p->lt; p->lv && l + 1 < p->nl; l++) {
    vc_lev *L = &p->lv[l];
    if (L->W.col) amgd_free(L->W.col);
    if (L->AfP.col) amgd_free(L->AfP.col);
    if (L->Wt) { amgd_free(L->Wt->ro); amgd_free(L->Wt->col); amgd_free(L->Wt->a); }
  }
  for (uint32_t l = 0; p->pl && l < p->lt; l++) {
    vc_plev *P = &p->pl[l];
    if (P->L.W.col) amgd_free(P->L.W.col);
    if (P->L.AfP.col) amgd_free(P->L.AfP.col);
    if (P->Wt && P->Wt->m) { amgd_free(P->Wt->m->ro); amgd_free(P->Wt->m->col); amgd_free(P->Wt->m->a); }
    if (P->cmap) amgd_free(P->cmap);
    halo_free(&P->hb); halo_free(&P->hx); halo_free(&P->hc);
  }
  for (uint32_t k = 0; p->gath && k < 3 * p->nl; k++)
    if (p->gath[k]) { amgd_free(p->gath[k]->ro); amgd_free(p->gath[k]->col); amgd_free(p->gath[k]->a); }
  halo_free(&p->h0);
  if (p->sbuf) amgd_free(p->sbuf);
  if (p->rbuf) amgd_free(p->rbuf);
  if (p->pos0) amgd_free(p->pos0);
  if (p->b) amgd_free(p->b);
  if (p->x) amgd_free(p->x);
  if (p->c0) amgd_free(p->c0);
  if (p->c1) amgd_free(p->c1);
  if (p->r) amgd_free(p->r);
  if (p->nb) amgd_free(p->nb);
  if (p->nx) amgd_free(p->nx);
  if (p->nc0) amgd_free(p->nc0);
  if (p->nc1) amgd_free(p->nc1);
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
static uint32_t lev_rows(const amgd_hier *h, uint32_t l) { return h->part ? h->lv[l].Pn->n : h->lv[l].A.d->rn; }
static uint32_t lev_nf(const amgd_hier *h, uint32_t l) { return h->part ? h->lv[l].Pf->n : h->lv[l].Af.d->rn; }
/* sizes, offsets and the positions of every level (whole vc vectors: the same on every rank);
   returns the largest F count, 0 on a malformed hierarchy */
static uint32_t plan_layout(struct amgd_vc_plan *p, const amgd_hier *h) {
  const uint32_t nl = p->nl = h->nlevels;
  p->lv = (vc_lev *)calloc(nl, sizeof(vc_lev));
  p->hpos = (uint32_t **)calloc(nl, sizeof(uint32_t *));
  uint32_t off = 0, maxnf = 1;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    vc_lev *L = &p->lv[l];
    L->nf = lev_nf(h, l);
    L->off = off;
    off += L->nf;
    if (L->nf > maxnf) maxnf = L->nf;
    if (lev_rows(h, l) != L->nf + lev_rows(h, l + 1)) { amgd_set_error("amgd_solve: level sizes do not add up"); return 0; }
  }
  if (lev_rows(h, nl - 1) != 1 || off + 1 != h->n0) { amgd_set_error("amgd_solve: the hierarchy does not end in a 1 x 1 level"); return 0; }
  const uint32_t N = p->N = off + 1;
  for (uint32_t l = 0; l + 1 < nl; l++) p->lv[l].nc = N - p->lv[l].off - p->lv[l].nf;
  /* positions, bottom up: pos_l[F] = off[l] + 0..nf-1, pos_l[C] = pos_{l+1} */
  p->hpos[nl - 1] = (uint32_t *)malloc(4);
  p->hpos[nl - 1][0] = N - 1;
  for (uint32_t l = nl - 1; l-- > 0;) {
    const uint32_t n = lev_rows(h, l);
    uint8_t *vc = (uint8_t *)malloc((size_t)n + 1);
    amgd_d2h(vc, h->lv[l].vc, n);
    uint32_t *pos = p->hpos[l] = (uint32_t *)malloc((size_t)n * 4 + 4);
    uint32_t kf = 0, kc = 0;
    const uint32_t ncn = lev_rows(h, l + 1);
    int ok = 1;
    for (uint32_t i = 0; i < n && ok; i++) {
      if (vc[i]) { if (kc < ncn) pos[i] = p->hpos[l + 1][kc++]; else ok = 0; }
      else { if (kf < p->lv[l].nf) pos[i] = p->lv[l].off + kf++; else ok = 0; }
    }
    free(vc);
    if (!ok || kc != ncn || kf != p->lv[l].nf) { amgd_set_error("amgd_solve: a C/F mask does not match its level's sizes"); return 0; }
  }
  return maxnf;
}
/* the Chebyshev scalars of level l */
static void lev_scalars(vc_lev *L, const amgd_level *H) {
  const uint32_t m = H->m >= 1 ? (uint32_t)H->m : 1;
  L->steps = m - 1;
  L->beta = (double *)calloc(m, 8);
  L->gamma = (double *)calloc(m, 8);
  cheb_scalars(H->rho, m, L->beta, L->gamma);
}
/* level l from whole matrices: renumbered columns, W', scalars, shapes */
static void lev_build(struct amgd_vc_plan *p, uint32_t l, const amgd_level *H, const dcsr *Af, const dcsr *W,
                      const dcsr *AfP, uint32_t rows_next) {
  vc_lev *L = &p->lv[l];
  const uint32_t off_next = L->off + L->nf;
  uint32_t *dpos = (uint32_t *)amgd_alloc((size_t)rows_next * 4 + 4);
  amgd_h2d(dpos, p->hpos[l + 1], (size_t)rows_next * 4);
  L->W = *W;
  L->W.col = NULL;
  L->AfP = *AfP;
  L->AfP.col = NULL;
  L->W.col = remap(W, dpos, off_next);
  L->AfP.col = remap(AfP, dpos, off_next);
  amgd_free(dpos);
  L->Wt = amgd_transpose(&L->W, NULL);
  L->Af = Af;
  L->D = H->D;
  lev_scalars(L, H);
  lev_shapes(L);
}
/* work vectors, the level-0 map, the bottom scalar (a0: the 1 x 1 level's value), the bytes */
static void plan_finish(struct amgd_vc_plan *p, const amgd_hier *h, uint32_t maxnf, uint32_t rlen, double a0) {
  const uint32_t nl = p->nl, N = p->N;
  p->pos0 = (uint32_t *)amgd_alloc((size_t)N * 4 + 4);
  amgd_h2d(p->pos0, p->hpos[0], (size_t)N * 4);
  for (uint32_t l = 0; l < nl; l++) { free(p->hpos[l]); p->hpos[l] = NULL; }
  free(p->hpos);
  p->hpos = NULL;
  p->b = dalloc(N); p->x = dalloc(N); p->ones = dones(N);
  p->c0 = dalloc(maxnf); p->c1 = dalloc(maxnf); p->r = dalloc(rlen);
  /* x = d*b with d = 0 on a null space, else 1./a (amg_setup.c:441-450) */
  p->dbot = h->nullspace != 0 ? 0. : 1. / a0;
  p->dbotv = dalloc(1);
  amgd_h2d(p->dbotv, &p->dbot, 8);
  /* the tail: the levels from the first whose slice [off[l], N) fits one workgroup */
  p->tail_first = nl - 1;
  p->tail_rows = 0;
  /* algorithmic bytes of one cycle (partitioned: of this rank's rows and the replicated
     levels): 12 B per entry of each matrix pass, 8 B per vector element read or written; in
     and out of the level-ordered layout: 4 N elements */
  p->bytes = 4ull * 8 * N;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const vc_lev *L = l < p->lt ? &p->pl[l].L : &p->lv[l];
    const uint64_t nf = L->nf, nc = p->lv[l].nc, st = L->steps;
    p->bytes += 12 * (L->Wt->nnz + L->W.nnz + L->AfP.nnz + st * L->Af->nnz);
    p->mbytes += 12 * (L->Wt->nnz + L->W.nnz + L->AfP.nnz + st * L->Af->nnz);
    p->bytes += 8 * (nf + 2 * nc);                         /* restriction: bF, bC in and out */
    p->bytes += 8 * (nc + 5 * nf);                         /* xc; xf, bf in and out, D, c */
    p->bytes += 8 * st * 4 * nf + (st > 1 ? 8 * (st - 1) * nf : 0) + (st ? 16 * nf : 0);
  }
}
static int plan_body(void *arg) {
  plan_args *pa = (plan_args *)arg;
  const amgd_hier *h = pa->h;
  const uint32_t nl = h->nlevels;
  struct amgd_vc_plan *p = (struct amgd_vc_plan *)calloc(1, sizeof *p);
  pa->p = p;
  const uint32_t maxnf = plan_layout(p, h);
  if (!maxnf) return -1;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const amgd_level *H = &h->lv[l];
    lev_build(p, l, H, H->Af.d, H->W.d, H->AfP.d, h->lv[l + 1].A.d->rn);
  }
  double a0 = 0;
  if (h->lv[nl - 1].A.d->nnz) amgd_d2h(&a0, h->lv[nl - 1].A.d->a, 8);
  plan_finish(p, h, maxnf, maxnf, a0);
  return 0;
}

/* ---- the partitioned plan ---- */
static int owner_of(const uint32_t *split, int np, uint32_t i) {
  int lo = 0, hi = np;                     /* split[lo] <= i < split[lo + 1] (empty ranges skipped) */
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (split[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}
/* the rank that owns position q < off[lt] */
static int pos_owner(const struct amgd_vc_plan *p, const amgd_hier *h, uint32_t q) {
  uint32_t l = 0;
  while (l + 1 < p->lt && q >= p->lv[l + 1].off) l++;
  return owner_of(h->lv[l].Pf->split, p->np, q - p->lv[l].off);
}
/* marks the device columns of M, shifted by base */
static void mark_cols(uint8_t *mark, const uint32_t *dcol, uint64_t nnz, uint32_t base) {
  if (!nnz) return;
  uint32_t *c = (uint32_t *)malloc(nnz * 4);
  amgd_d2h(c, dcol, nnz * 4);
  for (uint64_t k = 0; k < nnz; k++) mark[base + c[k]] = 1;
  free(c);
}
/* the marked entries of [lo, hi) that another rank owns, grouped by owner (ascending inside a
   group); own[q]: this rank holds q already.  idx_out: + shift.  Returns the list, cnt[np] filled */
typedef struct { uint32_t *idx; uint64_t n; } need_t;
static need_t need_list(const struct amgd_vc_plan *p, const amgd_hier *h, const uint8_t *mark, uint32_t lo,
                        uint32_t hi, const uint32_t *split, uint32_t shift, uint64_t *cnt) {
  const int np = p->np;
  need_t nd = {NULL, 0};
  for (int r = 0; r < np; r++) cnt[r] = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t *at = (uint64_t *)calloc((size_t)np + 1, 8);
    if (pass) {
      for (int r = 0; r < np; r++) at[r + 1] = at[r] + cnt[r];
      nd.n = at[np];
      nd.idx = (uint32_t *)malloc(nd.n * 4 + 4);
    }
    for (uint32_t q = lo; q < hi; q++) {
      if (!mark[q]) continue;
      const int o = split ? owner_of(split, np, q) : pos_owner(p, h, q);
      if (o == p->me) continue;
      if (pass) nd.idx[at[o]++] = q + shift; else cnt[o]++;
    }
    free(at);
  }
  return nd;
}
#define CNT(q, k) (cnt + ((size_t)(q) * K + (k)) * np)
/* K halo lists from their needs (grouped by owner; cnt: this rank's counts filled in): one
   count round, one request round, then per list the owners' send lists and the offsets.
   Collective: every rank calls it with the same K. */
static void halos_build(int np, int me, uint32_t K, const need_t *need, uint64_t *cnt, vc_halo *const *Hs,
                        uint64_t *maxs, uint64_t *maxr) {
  amgd_pcomm_allgather_u64(cnt, (int)(K * np));
  /* requests: to peer r the lists' groups for r, list after list; from peer q likewise */
  uint64_t *so = (uint64_t *)calloc((size_t)np + 1, 8), *ro = (uint64_t *)calloc((size_t)np + 1, 8);
  for (int r = 0; r < np; r++) {
    uint64_t s = 0, g = 0;
    for (uint32_t k = 0; k < K; k++) { s += CNT(me, k)[r]; g += CNT(r, k)[me]; }
    so[r + 1] = so[r] + 4 * s;
    ro[r + 1] = ro[r] + 4 * g;
  }
  uint32_t *hs = (uint32_t *)malloc(so[np] + 4), *hr = (uint32_t *)malloc(ro[np] + 4);
  {
    uint64_t *gat = (uint64_t *)calloc(K, 8);        /* where list k's group for the next peer starts */
    uint64_t w = 0;
    for (int r = 0; r < np; r++)
      for (uint32_t k = 0; k < K; k++) {
        const uint64_t c = CNT(me, k)[r];
        memcpy(hs + w, need[k].idx + gat[k], c * 4);
        gat[k] += c;
        w += c;
      }
    free(gat);
  }
  uint32_t *ds = (uint32_t *)amgd_alloc(so[np] + 8), *dr = (uint32_t *)amgd_alloc(ro[np] + 8);
  amgd_h2d(ds, hs, so[np]);
  amgd_pcomm_alltoallv(ds, so, dr, ro);
  amgd_d2h(hr, dr, ro[np]);
  amgd_free(ds); amgd_free(dr);
  for (uint32_t k = 0; k < K; k++) {
    vc_halo *H = Hs[k];
    H->soff = (uint64_t *)calloc((size_t)np + 1, 8);
    H->roff = (uint64_t *)calloc((size_t)np + 1, 8);
    for (int q = 0; q < np; q++) {
      H->soff[q + 1] = H->soff[q] + 8 * CNT(q, k)[me];
      H->roff[q + 1] = H->roff[q] + 8 * CNT(me, k)[q];
      for (int r = 0; r < np; r++) H->total += CNT(q, k)[r];
    }
    H->nsend = H->soff[np] / 8;
    H->nrecv = H->roff[np] / 8;
    uint32_t *si = (uint32_t *)malloc(H->nsend * 4 + 4);
    uint64_t w = 0;
    for (int q = 0; q < np; q++) {                    /* list k's part of what q sent */
      uint64_t at = ro[q] / 4;
      for (uint32_t j = 0; j < k; j++) at += CNT(q, j)[me];
      memcpy(si + w, hr + at, CNT(q, k)[me] * 4);
      w += CNT(q, k)[me];
    }
    H->sidx = (uint32_t *)amgd_alloc(H->nsend * 4 + 4);
    H->ridx = (uint32_t *)amgd_alloc(H->nrecv * 4 + 4);
    amgd_h2d(H->sidx, si, H->nsend * 4);
    amgd_h2d(H->ridx, need[k].idx, H->nrecv * 4);
    free(si);
    if (H->nsend > *maxs) *maxs = H->nsend;
    if (H->nrecv > *maxr) *maxr = H->nrecv;
  }
  free(so); free(ro); free(hs); free(hr);
}
static int pplan_body(void *arg) {
  plan_args *pa = (plan_args *)arg;
  const amgd_hier *h = pa->h;
  const uint32_t nl = h->nlevels;
  struct amgd_vc_plan *p = (struct amgd_vc_plan *)calloc(1, sizeof *p);
  pa->p = p;
  p->part = 1;
  const int np = p->np = amgd_pcomm_size(), me = p->me = amgd_pcomm_rank();
  if (h->lv[0].Pn->N != np) { amgd_set_error("amgd_solve: the hierarchy was set up on another communicator"); return -1; }
  const uint32_t maxnf = plan_layout(p, h);
  if (!maxnf) return -1;
  const uint32_t N = p->N;
  p->r0 = h->lv[0].Pn->split[me];
  p->r1 = h->lv[0].Pn->split[me + 1];
  /* lt: the first level whose slice has at most repl positions; the bottom level always */
  p->repl = repl_rows();
  uint32_t lt = nl - 1;
  for (uint32_t l = 0; l + 1 < nl; l++) if ((uint64_t)N - p->lv[l].off <= p->repl) { lt = l; break; }
  p->lt = lt;
  p->pl = (vc_plev *)calloc(lt + 1, sizeof(vc_plev));
  p->gath = (dcsr **)calloc(3 * (size_t)nl, sizeof(dcsr *));
  uint32_t maxc = 0;
  /* distributed levels: this rank's rows */
  for (uint32_t l = 0; l < lt; l++) {
    const amgd_level *H = &h->lv[l];
    vc_plev *P = &p->pl[l];
    vc_lev *L = &P->L;
    const uint32_t off_next = p->lv[l].off + p->lv[l].nf, rows_next = lev_rows(h, l + 1);
    const uint32_t c0 = h->lv[l + 1].Pn->split[me], c1 = h->lv[l + 1].Pn->split[me + 1];
    P->f0 = H->Pf->split[me];
    L->nf = H->Pf->split[me + 1] - P->f0;
    L->nc = p->lv[l].nc;
    L->off = p->lv[l].off;
    uint32_t *dpos = (uint32_t *)amgd_alloc((size_t)rows_next * 4 + 4);
    amgd_h2d(dpos, p->hpos[l + 1], (size_t)rows_next * 4);
    L->W = *H->W.p->m;
    L->W.col = NULL;
    L->AfP = *H->AfP.p->m;
    L->AfP.col = NULL;
    L->W.col = remap(H->W.p->m, dpos, off_next);
    L->AfP.col = remap(H->AfP.p->m, dpos, off_next);
    amgd_free(dpos);
    if (c1 - c0 > maxc) maxc = c1 - c0;
    P->cmap = (uint32_t *)amgd_alloc((size_t)(c1 - c0) * 4 + 4);
    amgd_h2d(P->cmap, p->hpos[l + 1] + c0, (size_t)(c1 - c0) * 4);
    P->Wt = pm_transpose(H->W.p);
    L->Wt = P->Wt->m;
    L->Af = H->Af.p->m;
    L->D = H->D + P->f0;
    lev_scalars(L, H);
    p->lv[l].steps = L->steps;
    lev_shapes(L);
    P->agoff = (uint64_t *)malloc(((size_t)np + 1) * 8);
    for (int r = 0; r <= np; r++) P->agoff[r] = 8ull * H->Pf->split[r];
  }
  /* replicated levels: whole matrices on every rank, the one-GPU level code */
  for (uint32_t l = lt; l + 1 < nl; l++) {
    const amgd_level *H = &h->lv[l];
    dcsr **G = &p->gath[3 * l];
    G[0] = pm_gather_full(H->Af.p);
    G[1] = pm_gather_full(H->W.p);
    G[2] = pm_gather_full(H->AfP.p);
    lev_build(p, l, H, G[0], G[1], G[2], lev_rows(h, l + 1));
  }
  double a0 = 0;
  {
    dcsr *B = pm_gather_full(h->lv[nl - 1].A.p);
    if (B->nnz) amgd_d2h(&a0, B->a, 8);
    dcsr_free(&B);
  }
  /* allgatherv offsets: b on the replicated slice (one buffer per level from lt, the bottom
     point last), x on the distributed levels, dx */
  const uint32_t nd = nl - lt;
  p->downoff = (uint64_t *)calloc((size_t)nd * (np + 1), 8);
  for (uint32_t l = lt; l < nl; l++)
    for (int r = 0; r <= np; r++)
      p->downoff[(size_t)(l - lt) * (np + 1) + r] = 8ull * (l + 1 < nl ? h->lv[l].Pf->split[r] : h->lv[l].Pn->split[r]);
  p->down_bytes = 8ull * (N - (lt + 1 < nl ? p->lv[lt].off : N - 1)) * (uint64_t)(np - 1);
  p->xoff = (uint64_t *)calloc((size_t)(lt + 1) * (np + 1), 8);
  for (uint32_t l = 0; l < lt; l++) memcpy(p->xoff + (size_t)l * (np + 1), p->pl[l].agoff, ((size_t)np + 1) * 8);
  p->x_bytes = lt ? 8ull * (lt + 1 < nl ? p->lv[lt].off : N - 1) * (uint64_t)(np - 1) : 0;
  p->dxoff = (uint64_t *)malloc(((size_t)np + 1) * 8);
  for (int r = 0; r <= np; r++) p->dxoff[r] = 8ull * h->lv[0].Pn->split[r];
  /* halo lists: per distributed level the entries of bF (W'), x (W and AfP) and c (Af) that
     the own rows reference and another rank owns; one count round and one request round
     for all of them.  Replicated positions are on every rank: never requested.  The last
     list serves the Krylov solvers' level-0 product (amgd_krylov.c): the entries of a whole
     level-0 vector that the own rows of A reference, in the same two rounds. */
  if (np > 1) {
    const uint32_t K = 3 * lt + 1, xtop = lt ? p->lv[lt - 1].off + p->lv[lt - 1].nf : 0;   /* = off[lt] */
    uint8_t *mark = (uint8_t *)malloc((size_t)N + 1);
    need_t *need = (need_t *)calloc(K, sizeof(need_t));
    uint64_t *cnt = (uint64_t *)calloc((size_t)np * K * np, 8);
    for (uint32_t l = 0; l < lt; l++) {
      const vc_plev *P = &p->pl[l];
      const uint32_t nf = p->lv[l].nf, off = p->lv[l].off, off_next = off + nf;
      const uint32_t *fs = h->lv[l].Pf->split;
      memset(mark, 0, (size_t)nf + 1);
      mark_cols(mark, P->L.Wt->col, P->L.Wt->nnz, 0);
      need[3 * l] = need_list(p, h, mark, 0, nf, fs, off, CNT(me, 3 * l));
      memset(mark, 0, (size_t)N + 1);
      mark_cols(mark, P->L.W.col, P->L.W.nnz, off_next);
      mark_cols(mark, P->L.AfP.col, P->L.AfP.nnz, off_next);
      need[3 * l + 1] = need_list(p, h, mark, off_next, xtop, NULL, 0, CNT(me, 3 * l + 1));
      memset(mark, 0, (size_t)nf + 1);
      mark_cols(mark, P->L.Af->col, P->L.Af->nnz, 0);
      need[3 * l + 2] = need_list(p, h, mark, 0, nf, fs, 0, CNT(me, 3 * l + 2));
    }
    {
      const dcsr *A0 = h->lv[0].A.p->m;
      memset(mark, 0, (size_t)N + 1);
      mark_cols(mark, A0->col, A0->nnz, 0);
      need[K - 1] = need_list(p, h, mark, 0, N, h->lv[0].Pn->split, 0, CNT(me, K - 1));
    }
    free(mark);
    vc_halo **Hs = (vc_halo **)malloc(K * sizeof *Hs);
    for (uint32_t k = 0; k + 1 < K; k++) {
      vc_plev *P = &p->pl[k / 3];
      Hs[k] = k % 3 == 0 ? &P->hb : k % 3 == 1 ? &P->hx : &P->hc;
    }
    Hs[K - 1] = &p->h0;
    uint64_t maxs = 0, maxr = 0;
    halos_build(np, me, K, need, cnt, Hs, &maxs, &maxr);
    free(Hs);
    for (uint32_t k = 0; k < K; k++) free(need[k].idx);
    free(need); free(cnt);
    p->sbuf = dalloc(maxs);
    p->rbuf = dalloc(maxr);
  }
  /* r also takes the composed restriction's sums of the own C rows */
  plan_finish(p, h, maxnf, maxnf > maxc ? maxnf : maxc, a0);
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
  for (uint32_t l = p->nl - 1; l-- > p->lt;) {
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

/* levels l0 .. of the cycle on whole matrices (one GPU: l0 = 0; partitioned: the replicated levels) */
static void cycle_from(struct amgd_vc_plan *p, uint32_t l0) {
  const int fused = fused_on();
  const uint32_t nl = p->nl, N = p->N;
  uint32_t tf = p->tail ? p->tail_first : nl - 1;
  for (uint32_t l = l0; l < tf; l++) {
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
  for (uint32_t l = tf; l-- > l0;) {
    const vc_lev *L = &p->lv[l];
    vc_up(L, p->x + L->off + L->nf, p->x + L->off, p->b + L->off, p->c0, p->c1, p->r, fused, NULL);
  }
}

/* ---- the partitioned cycle ---- */
/* collectives and bytes all ranks send in the cycle running, from the plan's counts */
static uint64_t g_pc_coll, g_pc_bytes;
API void amgd_solve_comm_stats(uint64_t *collectives, uint64_t *bytes_sent) {
  if (collectives) *collectives = g_pc_coll;
  if (bytes_sent) *bytes_sent = g_pc_bytes;
}
/* one halo exchange: the peers' entries packed by send list, one alltoallv, the received
   entries scattered to their places */
static void halo_run(const vc_halo *H, double *v, double *sbuf, double *rbuf) {
  amgd_vc_pack(sbuf, v, H->sidx, H->nsend);
  amgd_pcomm_alltoallv(sbuf, H->soff, rbuf, H->roff);
  amgd_vc_unpack(v, H->ridx, rbuf, H->nrecv);
}
/* Completes on this rank the entries of v that its rows are about to read: the halo list's
   (pack, alltoallv, unpack) or the whole F segment seg of nf entries (allgatherv).  Entered
   by every rank or by none: np, the list's global count and nf are the same on all. */
static void exchange(struct amgd_vc_plan *p, const vc_halo *H, double *v, double *seg, uint32_t nf,
                     const uint64_t *agoff) {
  if (p->np == 1) return;
  if (halo_on()) {
    if (!H->total) return;
    amgd_route_hit(AMGD_R_VC_HALO);
    g_launches += 2;
    halo_run(H, v, p->sbuf, p->rbuf);
    g_pc_bytes += 8 * H->total;
  } else {
    if (!seg || !nf) return;
    amgd_route_hit(AMGD_R_VC_ALLG);
    void *buf = seg;
    amgd_allgatherv(1, &buf, agoff);
    g_pc_bytes += 8ull * nf * (uint64_t)(p->np - 1);
  }
  g_pc_coll++;
}
/* mode 0 composed, 1 thread per row, 2 cooperative: b[map[c]] += row c of Wt times bF */
void amgd_vc_restrict_map_run(const dcsr *Wt, const double *bF, double *b, const uint32_t *map, int mode) {
  if (Wt->rn) {
    double *r = mode ? NULL : dalloc(Wt->rn);
    restrict_as(mode == 1 ? VC_THR : mode == 2 ? VC_COOP : VC_COMP, Wt, bF, b, map, r);
    amgd_free(r);
  }
  amgd_sync();
}
/* the halo exchange on its own (amgd_testapi.c): M holds this rank's rows, its columns index v
   (n entries, owned by split); afterwards v holds the owners' values at every referenced entry */
void amgd_vc_halo_test(const dcsr *M, const uint32_t *split, uint32_t n, double *v) {
  struct amgd_vc_plan fake;
  memset(&fake, 0, sizeof fake);
  const int np = fake.np = amgd_pcomm_size(), me = fake.me = amgd_pcomm_rank();
  uint8_t *mark = (uint8_t *)calloc((size_t)n + 1, 1);
  mark_cols(mark, M->col, M->nnz, 0);
  uint64_t *cnt = (uint64_t *)calloc((size_t)np * np, 8);
  need_t need = need_list(&fake, NULL, mark, 0, n, split, 0, cnt + (size_t)me * np);
  free(mark);
  vc_halo H, *Hp = &H;
  memset(&H, 0, sizeof H);
  uint64_t maxs = 0, maxr = 0;
  halos_build(np, me, 1, &need, cnt, &Hp, &maxs, &maxr);
  free(need.idx); free(cnt);
  double *sb = dalloc(maxs), *rb = dalloc(maxr);
  if (H.total) halo_run(&H, v, sb, rb);
  amgd_sync();
  amgd_free(sb); amgd_free(rb);
  halo_free(&H); halo_free_host(&H);
}
typedef struct { struct amgd_vc_plan *p; uint32_t l; } cx_ctx;
static void c_exchange(void *ctx, double *c) {
  const cx_ctx *x = (const cx_ctx *)ctx;
  const vc_plev *P = &x->p->pl[x->l];
  exchange(x->p, &P->hc, c, c, x->p->lv[x->l].nf, P->agoff);
}
/* bC += W' bF on the own C rows: b[cmap[c]] += the row's sum, left to right from its start */
static void vc_restrict_rows(const vc_plev *P, const double *bF, double *b, double *r, int fused) {
  const vc_lev *L = &P->L;
  if (!L->Wt->rn) return;
  const int f = form(L->sh_r, fused);
  form_hit(f);
  g_launches += f != VC_COMP ? 1 : 2;
  restrict_as(f, L->Wt, bF, b, P->cmap, r);
}
static void pcycle(struct amgd_vc_plan *p) {
  const int fused = fused_on();
  const uint32_t nl = p->nl, lt = p->lt;
  for (uint32_t l = 0; l < lt; l++) {
    const vc_plev *P = &p->pl[l];
    const uint32_t off = p->lv[l].off;
    exchange(p, &P->hb, p->b, p->b + off, p->lv[l].nf, P->agoff);
    vc_restrict_rows(P, p->b + off, p->b, p->r, fused);
  }
  if (p->np > 1) {                         /* b on the replicated slice, from its owners */
    void **bufs = (void **)malloc((size_t)(nl - lt) * sizeof(void *));
    for (uint32_t l = lt; l < nl; l++) bufs[l - lt] = p->b + (l + 1 < nl ? p->lv[l].off : p->N - 1);
    amgd_allgatherv((int)(nl - lt), bufs, p->downoff);
    free(bufs);
    g_pc_coll++;
    g_pc_bytes += p->down_bytes;
  }
  if (lt + 1 < nl) amgd_route_hit(AMGD_R_VC_REPL);
  cycle_from(p, lt);
  for (uint32_t l = lt; l-- > 0;) {
    const vc_plev *P = &p->pl[l];
    const uint32_t off = p->lv[l].off, nf = p->lv[l].nf;
    /* allgather mode: the next level's F segment, when its owners computed it (below it x is whole) */
    exchange(p, &P->hx, p->x, l + 1 < lt ? p->x + off + nf : NULL, l + 1 < lt ? p->lv[l + 1].nf : 0,
             l + 1 < lt ? p->pl[l + 1].agoff : NULL);
    cx_ctx cx = {p, l};
    const vc_rows X = {P->f0, c_exchange, &cx};
    vc_up(&P->L, p->x + off + nf, p->x + off + P->f0, p->b + off + P->f0, p->c0, p->c1, p->r, fused, &X);
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

API int amgd_hier_rows(const amgd_hier *h, uint32_t *r0, uint32_t *r1) {
  if (!h || h->nlevels == 0) return -1;
  const int me = h->part ? amgd_pcomm_rank() : 0;
  if (h->part && h->lv[0].Pn->N != amgd_pcomm_size()) return -1;
  if (r0) *r0 = h->part ? h->lv[0].Pn->split[me] : 0;
  if (r1) *r1 = h->part ? h->lv[0].Pn->split[me + 1] : h->n0;
  return 0;
}

static int solve_device(amgd_hier *h, double *dx, const double *db, int flags);
static int solve_rows(amgd_hier *h, double *xo, const double *bo, double *dx, int flags);
/* the partitioned cycle on own-row vectors (amgd_krylov.c): bo and xo hold this rank's level-0
   rows alone, r1 - r0 entries from their bases; collective, flags bit 0 as amgd_solve_device */
int amgd_vc_solve_own(amgd_hier *h, double *xo, const double *bo, int flags) {
  const int was = amgd_comm_part_get();
  amgd_comm_part_set(1);
  int rc = amgd_vc_prepare(h);
  if (rc == 0) rc = solve_rows(h, xo, bo, NULL, flags & 1);
  amgd_comm_part_set(was);
  return rc;
}
API int amgd_solve_device(amgd_hier *h, double *dx, const double *db, int flags) {
  if (!h || h->nlevels == 0 || h->n0 == 0 || !dx || !db) return -1;
  if (!h->part) return solve_device(h, dx, db, flags);
  /* the partitioned call reads and writes a rank's own rows only and is collective: a caller
     says so with flag bit 2; without it a partitioned hierarchy is refused as before */
  if (!(flags & 4)) return -3;
  /* a partitioned hierarchy is solved in partitioned mode whatever the communicator's flag
     says now (crs_setup restores it after the setup): no kernel row-shards a rank's block */
  const int was = amgd_comm_part_get();
  amgd_comm_part_set(1);
  const int rc = solve_device(h, dx, db, flags);
  amgd_comm_part_set(was);
  return rc;
}
/* the plan of h, built on the first solve */
static int plan_ensure(amgd_hier *h) {
  /* a plan made for another replication limit is rebuilt (every rank reads the same limit) */
  if (h->plan && h->plan->part && h->plan->repl != repl_rows()) amgd_vc_plan_free(&h->plan);
  if (!h->plan) {
    plan_args a = {h, NULL};
    const int rc = amgd_try(h->part ? pplan_body : plan_body, &a);
    if (rc != 0) {
      if (rc == -2) amgd_vc_plan_free_host(&a.p);     /* device blocks: released by the unwind */
      else amgd_vc_plan_free(&a.p);
      return rc == -2 ? -2 : -1;
    }
    h->plan = a.p;
  }
  return 0;
}
int amgd_vc_prepare(amgd_hier *h) {
  const int prc = plan_ensure(h);
  if (prc != 0) return prc;
  struct amgd_vc_plan *p = h->plan;
  tail_args ta = {h};
  if (amgd_try(tail_body, &ta) != 0) { p->tail = NULL; p->tail_set = 0; p->tail_first = p->nl - 1; return -2; }
  return 0;
}
static int solve_device(amgd_hier *h, double *dx, const double *db, int flags) {
  const int prc = amgd_vc_prepare(h);
  if (prc != 0) return prc;
  const uint32_t r0 = h->plan->part ? h->plan->r0 : 0;
  return solve_rows(h, dx + r0, db + r0, dx, flags);
}
/* one cycle: bo and xo start at this rank's first level-0 row (one GPU: the whole vectors), dx
   is the whole output that flag bit 1 completes on a partitioned hierarchy */
static int solve_rows(amgd_hier *h, double *xo, const double *bo, double *dx, int flags) {
  struct amgd_vc_plan *p = h->plan;
  /* the setup's event timers (the long-row SpMV's slots) stay off inside a cycle: only a
     setup's statistics read them, so a solve must not queue events on them */
  amgd_xtimer_begin(AMGD_XT_VC);
  amgd_timers_enable(0);
  g_pc_coll = g_pc_bytes = 0;
  if (p->part) {
    /* only the own rows of db are read, only the own rows of dx written (flag 2: all of dx) */
    amgd_vc_scatter(p->b, bo, p->pos0 + p->r0, p->r1 - p->r0);
    pcycle(p);
  } else {
    amgd_vc_scatter(p->b, bo, p->pos0, p->N);
    cycle_from(p, 0);
  }
  amgd_timers_enable(1);
  amgd_xtimer_end(AMGD_XT_VC);
  g_launches += 2;                                     /* into and out of the level-ordered layout */
  g_cycles++;
  g_bytes_last = p->bytes;
  double avg = 0;
  if (flags & 1) {
    /* x -= (1/n) sum(x), the sum left to right in the level-ordered layout (amg.c:181-184);
       partitioned: the sequential sum needs the whole x, so the distributed levels' F
       segments are completed on every rank first (one allgatherv, 8 B per such position) */
    if (p->part && p->np > 1 && p->lt > 0) {
      void **bufs = (void **)malloc((size_t)p->lt * sizeof(void *));
      for (uint32_t l = 0; l < p->lt; l++) bufs[l] = p->x + p->lv[l].off;
      amgd_allgatherv((int)p->lt, bufs, p->xoff);
      free(bufs);
      g_pc_coll++;
      g_pc_bytes += p->x_bytes;
    }
    sum_args sa = {p, 0.};
    const int ex = amgd_get_exact();
    amgd_set_exact(1);
    const int rc = amgd_try(sum_body, &sa);
    amgd_set_exact(ex);
    if (rc != 0) return -2;
    const double tni = 1. / (double)p->N;
    avg = tni * sa.sum;
  }
  if (p->part) {
    amgd_vc_gather(xo, p->x, p->pos0 + p->r0, p->r1 - p->r0, flags & 1, avg);
    if ((flags & 2) && dx && p->np > 1) {
      void *buf = dx;
      amgd_allgatherv(1, &buf, p->dxoff);
      g_pc_coll++;
      g_pc_bytes += 8ull * p->N * (uint64_t)(p->np - 1);
    }
  } else {
    amgd_vc_gather(xo, p->x, p->pos0, p->N, flags & 1, avg);
  }
  return 0;
}

/* ---- what the Krylov solver needs of a partitioned plan (amgd_krylov.c) ---- */
/* ranks, this rank, its level-0 rows, the byte offsets of the level-0 rows by rank */
void amgd_vc_part_info(const amgd_hier *h, int *np, int *me, uint32_t *r0, uint32_t *r1, const uint64_t **rowoff) {
  const struct amgd_vc_plan *p = h->plan;
  *np = p->np; *me = p->me; *r0 = p->r0; *r1 = p->r1; *rowoff = p->dxoff;
}
/* 1: a level-0 product is preceded by an exchange in the mode in force -- decided from the
   global counts, the same on every rank */
int amgd_vc_a0_has_exchange(const amgd_hier *h) {
  const struct amgd_vc_plan *p = h->plan;
  if (p->np == 1) return 0;
  return halo_on() ? p->h0.total != 0 : p->N != 0;
}
/* completes on this rank the entries of the whole level-0 vector v that its rows of A read
   (v valid on the own rows): the halo list's, or every rank's segment.  Returns the
   collectives made (0 or 1), *bytes += what all ranks sent */
int amgd_vc_a0_exchange(amgd_hier *h, double *v, uint64_t *bytes) {
  struct amgd_vc_plan *p = h->plan;
  const uint64_t c = g_pc_coll, b = g_pc_bytes;
  exchange(p, &p->h0, v, v, p->N, p->dxoff);
  const int ran = (int)(g_pc_coll - c);
  *bytes += g_pc_bytes - b;
  g_pc_coll = c;
  g_pc_bytes = b;
  return ran;
}
/* the product on a rank's rows with its halo exchange, on its own (amgd_testapi.c): M holds
   this rank's rows, its columns index v (n entries, owned by split, valid on the own ones);
   z = M v after the exchange, v as the exchange left it */
void amgd_vc_spmv_part_test(const dcsr *M, const uint32_t *split, uint32_t n, double *v, double *z) {
  amgd_vc_halo_test(M, split, n, v);
  if (M->rn) amgd_spmv(M, v, z, 0., NULL, 1., NULL);
  amgd_sync();
}

/* ------------------------------------------------------------------------ */
/* several right-hand sides (DESIGN.md "Solve", the multi-RHS part)          */
/* ------------------------------------------------------------------------ */
/* nrhs columns run in groups of K = 8, 4 or 2, greedily, each group ONE pass over the
   hierarchy: inside a group the level-ordered vectors are interleaved, element (position q,
   column j) at q*K + j, so the positions -- pos0, the renumbered W / AfP, W' -- are the
   single-vector plan's and only the vectors' stride differs.  The loop is cycle_from's over
   the same vc_lev records and Chebyshev scalars with the same kernels over the K-column
   policies (amgd_solve.hip, amgd_vc_dev.h), per-level launches down to the bottom (no
   one-workgroup tail).  A column left over goes through the single-vector cycle.  A level
   whose matrix has an outlier row has no K-column form: its restriction or up-sweep runs
   column by column through the single-vector code on contiguous copies (the plan's own b
   and x), counted by vc_mr_comp;
   the other levels keep the K-column kernels.  Column j comes out bit for bit as
   amgd_solve_device gives it.  A group's columns are always a table of pointers (amgd.h), and
   one loop, amgd_vc_cycles_n, forms the groups for amgd_solve_device_n and for the lock-step
   Krylov solver (amgd_krylov.c).  The group sizes allowed by default: DESIGN.md, the measured
   table; vc_mrhs_k (AMGD_VC_MRHS_K=8,4,2, a list; 0: none) chooses others. */
static int mrhs_mask(void) { return (int)amgd_knob(AMGD_K_VC_MRHS_K) & (8 | 4 | 2); }
/* kernel family of a product of the given row shape: 0 short-row, 1 long-row (vc_mrhs_family:
   0 by row shape, 1 / 2 forced; the level hooks name theirs for one call) */
static int g_mr_fam_run = -1;
static int mr_fam(int shape) {
  const int64_t f = g_mr_fam_run >= 0 ? g_mr_fam_run : amgd_knob(AMGD_K_VC_MRHS_FAMILY);
  return f == 1 ? 0 : f == 2 ? 1 : shape == VC_COOP;
}
static void mr_hit(int fam) {
  amgd_route_hit(fam ? AMGD_R_VC_MR_WAVE : AMGD_R_VC_MR_THR);
  g_launches++;
}
static void vc_restrict_n(const vc_lev *L, int K, const double *bF, double *bC) {
  const int f = mr_fam(L->sh_r);
  mr_hit(f);
  amgd_vc_restrict(f, K, L->Wt, bF, bC, NULL);
}
/* vc_up for K interleaved columns; returns the buffer holding the last c */
static double *vc_up_n(const vc_lev *L, int K, const double *xc, double *xf, double *bf, double *c0, double *c1) {
  const int fp = mr_fam(L->sh_p), fc = mr_fam(L->sh_c);
  mr_hit(fp);
  amgd_vc_prolong(fp, K, &L->W, &L->AfP, L->D, xc, xf, bf, c0, L->steps == 0);
  double *c = c0, *cn = c1;
  for (uint32_t k = 0; k < L->steps; k++) {
    mr_hit(fc);
    amgd_vc_cheb(fc, K, L->Af, L->D, bf, c, c, cn, L->beta[k], L->gamma[k], k > 0, k + 1 == L->steps ? xf : NULL);
    double *t = c; c = cn; cn = t;
  }
  return c;
}
static int lev_has_comp(const vc_lev *L) {
  return L->sh_r == VC_COMP || L->sh_p == VC_COMP || (L->steps && L->sh_c == VC_COMP);
}
/* the matrix bytes (12 B per entry per pass) of the products cycle_n runs column by column */
static uint64_t comp_mbytes(const struct amgd_vc_plan *p) {
  uint64_t by = 0;
  for (uint32_t l = 0; l + 1 < p->nl; l++) {
    const vc_lev *L = &p->lv[l];
    if (L->sh_r == VC_COMP) by += 12 * L->Wt->nnz;
    if (L->sh_p == VC_COMP || (L->steps && L->sh_c == VC_COMP))
      by += 12 * (L->W.nnz + L->AfP.nnz + (uint64_t)L->steps * L->Af->nnz);
  }
  return by;
}
static void cycle_n(struct amgd_vc_plan *p, int K) {
  const int fused = fused_on();
  const uint32_t nl = p->nl, N = p->N;
  const uint64_t k = (uint64_t)K;
  for (uint32_t l = 0; l + 1 < nl; l++) {
    const vc_lev *L = &p->lv[l];
    if (L->sh_r != VC_COMP) {
      vc_restrict_n(L, K, p->nb + k * L->off, p->nb + k * (L->off + L->nf));
      continue;
    }
    for (int j = 0; j < K; j++) {          /* an outlier row in W': column by column */
      amgd_route_hit(AMGD_R_VC_MR_COMP);
      g_launches += 2;
      amgd_vcn_col(p->b + L->off, p->nb + k * L->off, L->nf + L->nc, K, j);
      vc_restrict(L, p->b + L->off, p->b + L->off + L->nf, fused);
      amgd_vcn_putcol(p->nb + k * (L->off + L->nf), p->b + L->off + L->nf, L->nc, K, j);
    }
  }
  g_launches++;
  amgd_vcn_bottom(p->nx + k * (N - 1), p->nb + k * (N - 1), p->dbot, K);   /* x = d*b (amg.c:130) */
  for (uint32_t l = nl - 1; l-- > 0;) {
    const vc_lev *L = &p->lv[l];
    if (L->sh_p != VC_COMP && !(L->steps && L->sh_c == VC_COMP)) {
      vc_up_n(L, K, p->nx + k * (L->off + L->nf), p->nx + k * L->off, p->nb + k * L->off, p->nc0, p->nc1);
      continue;
    }
    for (int j = 0; j < K; j++) {          /* an outlier row in W, AfP or Af */
      amgd_route_hit(AMGD_R_VC_MR_COMP);
      g_launches += 3;
      amgd_vcn_col(p->x + L->off + L->nf, p->nx + k * (L->off + L->nf), L->nc, K, j);
      amgd_vcn_col(p->b + L->off, p->nb + k * L->off, L->nf, K, j);
      vc_up(L, p->x + L->off + L->nf, p->x + L->off, p->b + L->off, p->c0, p->c1, p->r, fused, NULL);
      amgd_vcn_putcol(p->nx + k * L->off, p->x + L->off, L->nf, K, j);
    }
  }
}
typedef struct { struct amgd_vc_plan *p; uint32_t K; } nbuf_args;
static int nbuf_body(void *arg) {
  nbuf_args *a = (nbuf_args *)arg;
  struct amgd_vc_plan *p = a->p;
  const uint64_t n = (uint64_t)p->N * a->K;
  p->nb = dalloc(n); p->nx = dalloc(n); p->nc0 = dalloc(n); p->nc1 = dalloc(n);
  return 0;
}
/* one group, out->p[j] = cycle(in->p[j]), j < K: in, the cycle, the per-column mean, out */
static int group_n(struct amgd_vc_plan *p, const amgd_ptr8 *out, const amgd_cptr8 *in, int K, int flags) {
  /* as in solve_device: the setup's event timers stay off inside the cycle -- the levels that
     fall back column by column go through amgd_spmv, whose long-row kernel is timed on the
     setup's slots, which no solve reads */
  amgd_timers_enable(0);
  amgd_vcn_scatter(p->nb, in, p->pos0, p->N, K);
  cycle_n(p, K);
  amgd_timers_enable(1);
  g_launches += 2;
  double avg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (flags & 1) {
    /* the ordered sum needs a contiguous column: column j into the plan's x, then the
       single-vector cycle's exact dot against ones -- K small passes */
    const double tni = 1. / (double)p->N;
    for (int j = 0; j < K; j++) {
      amgd_vcn_col(p->x, p->nx, p->N, K, j);
      sum_args sa = {p, 0.};
      const int ex = amgd_get_exact();
      amgd_set_exact(1);
      const int rc = amgd_try(sum_body, &sa);
      amgd_set_exact(ex);
      if (rc != 0) return -2;
      avg[j] = tni * sa.sum;
    }
  }
  amgd_vcn_gather(out, p->nx, p->pos0, p->N, K, flags & 1, avg);
  return 0;
}
/* the interleaved work vectors for groups of up to kmax columns */
static int nbuf_ensure(struct amgd_vc_plan *p, uint32_t kmax) {
  if (kmax <= p->nk) return 0;
  if (p->nb) { amgd_free(p->nb); amgd_free(p->nx); amgd_free(p->nc0); amgd_free(p->nc1); }
  p->nb = p->nx = p->nc0 = p->nc1 = NULL;
  p->nk = 0;
  nbuf_args na = {p, kmax};
  if (amgd_try(nbuf_body, &na) != 0) { p->nb = p->nx = p->nc0 = p->nc1 = NULL; return -2; }
  p->nk = kmax;
  return 0;
}
int amgd_vc_mrhs_mask(void) { return mrhs_mask(); }
/* the size of the next group for `left` columns: the largest allowed one that fits, 0: a single column */
int amgd_vc_group_size(int mask, int left) {
  for (int K = 8; K >= 2; K >>= 1) if ((mask & K) && left >= K) return K;
  return 0;
}
/* out[q] = cycle(in[q]) for nc columns given by pointer, in greedy groups (their work vectors
   reserved); a leftover column takes the single-vector cycle and hits the route `single`.
   Bit for bit amgd_solve_device per column.  bytes, when given, grows by the cycles' traffic */
int amgd_vc_cycles_n(amgd_hier *h, int nc, const double *const *in, double *const *out, int flags, int single,
                     uint64_t *bytes) {
  struct amgd_vc_plan *p = h->plan;
  const int mask = mrhs_mask();
  uint64_t by = 0;
  for (int q = 0; q < nc;) {
    const int K = amgd_vc_group_size(mask, nc - q);
    int rc;
    if (!K) {
      amgd_route_hit(single);
      rc = solve_device(h, out[q], in[q], flags & 1);
      by += p->bytes;
      q++;
    } else {
      const amgd_cptr8 ti = amgd_cptr8_of(in + q, K);
      const amgd_ptr8 to = amgd_ptr8_of(out + q, K);
      rc = group_n(p, &to, &ti, K, flags);
      /* the matrices once per group -- but those of a level that fell back column by column
         once per column -- and the vectors per column */
      by += p->mbytes + (uint64_t)(K - 1) * comp_mbytes(p) + (uint64_t)K * (p->bytes - p->mbytes);
      q += K;
    }
    if (rc != 0) return rc;
  }
  if (bytes) *bytes += by;
  return 0;
}
static uint64_t g_n_calls, g_n_cols, g_n_bytes_last;
API int amgd_solve_device_n(amgd_hier *h, double *dX, const double *dB, int nrhs, uint64_t ld, int flags) {
  if (!h || h->nlevels == 0 || h->n0 == 0 || !dX || !dB || nrhs < 1 || ld < h->n0) return -1;
  if (h->part) return -3;
  const int prc = plan_ensure(h);
  if (prc != 0) return prc;
  if (nbuf_ensure(h->plan, (uint32_t)amgd_vc_group_size(mrhs_mask(), nrhs)) != 0) return -2;
  amgd_xtimer_begin(AMGD_XT_VCN);
  uint64_t bytes = 0;
  int rc = 0;
  /* 8 columns at a time: every group size divides 8, so the groups are the whole block's */
  for (int j = 0; j < nrhs && rc == 0; j += 8) {
    const int nc = nrhs - j < 8 ? nrhs - j : 8;
    const double *in[8];
    double *out[8];
    for (int q = 0; q < nc; q++) {
      in[q] = dB + (uint64_t)(j + q) * ld;
      out[q] = dX + (uint64_t)(j + q) * ld;
    }
    rc = amgd_vc_cycles_n(h, nc, in, out, flags, AMGD_R_VC_MR_SINGLE, &bytes);
  }
  amgd_xtimer_end(AMGD_XT_VCN);
  g_n_calls++;
  if (rc != 0) return rc;
  g_n_cols += (uint64_t)nrhs;
  g_n_bytes_last = bytes;
  return 0;
}
/* the plan of h exists (amgd_vc_prepare): its interleaved work vectors for groups of K columns */
int amgd_vc_mrhs_reserve(amgd_hier *h, int K) { return nbuf_ensure(h->plan, (uint32_t)K); }
/* N * (the largest group size reserved) doubles, free between two cycles */
double *amgd_vc_mrhs_scratch(const amgd_hier *h) { return h->plan->nb; }
/* the row shape of a level-0 product: 0 an outlier row (no K-column form), 1 short rows, 2 long rows */
int amgd_vc_mat_shape(const dcsr *M) { return mat_shape(M); }
API void amgd_solve_n_stats(uint64_t *calls, uint64_t *columns, double *ms, uint64_t *bytes) {
  if (calls) *calls = g_n_calls;
  if (columns) *columns = g_n_cols;
  if (ms) *ms = amgd_xtimer_ms(AMGD_XT_VCN);
  if (bytes) *bytes = g_n_bytes_last;
}

/* the plan of h's last solve, 4 values per level: first position, F points, matrix entries one
   cycle passes over (W', W, AfP, m - 1 times Af; a distributed level: this rank's rows only),
   1 when the level runs replicated.  Returns the levels written (tools/part_solve_counts.py) */
int amgd_vc_plan_levels(const amgd_hier *h, uint64_t *out, int cap) {
  const struct amgd_vc_plan *p = h ? h->plan : NULL;
  if (!p) return 0;
  int n = 0;
  for (uint32_t l = 0; l + 1 < p->nl && n < cap; l++, n++) {
    const int dist = p->part && l < p->lt;
    const vc_lev *L = dist ? &p->pl[l].L : &p->lv[l];
    out[4 * n] = p->lv[l].off;
    out[4 * n + 1] = p->lv[l].nf;
    out[4 * n + 2] = L->Wt->nnz + L->W.nnz + L->AfP.nnz + (uint64_t)L->steps * L->Af->nnz;
    out[4 * n + 3] = p->part && !dist;
  }
  return n;
}

API void amgd_solve_stats(uint64_t *cycles, double *ms, uint64_t *bytes) {
  if (cycles) *cycles = g_cycles;
  if (ms) *ms = amgd_xtimer_ms(AMGD_XT_VC);
  if (bytes) *bytes = g_bytes_last;
}
void amgd_vc_stats_reset(void) {
  amgd_xtimer_zero(AMGD_XT_VC);
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
    c = vc_up(&L, x + L.nf, x, b, c0, c1, r, mode, NULL);
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

/* ---- K columns (amgd_test_vc_level_n / _restrict_n) ---- */
/* X: K columns of nf + nc doubles (xf, then xc), B and C_out: K columns of nf, column-major on
   the device.  family: 0 by row shape, 1 short-row, 2 long-row kernels.  A level with an outlier
   row runs column by column through the single-vector kernels (vc_mr_comp counts them). */
int amgd_vc_level_run_n(const dcsr *Af, const dcsr *W, const dcsr *AfP, const double *D, uint32_t m, double rho,
                        double *X, double *B, double *C_out, int K, int family) {
  if (K != 2 && K != 4 && K != 8) return -1;
  vc_lev L;
  memset(&L, 0, sizeof L);
  L.nf = W->rn; L.nc = W->cn;
  L.steps = m ? m - 1 : 0;
  L.W = *W; L.AfP = *AfP; L.Af = Af; L.D = D;
  dcsr none = {0, 0, 0, NULL, NULL, NULL};
  L.Wt = &none;
  lev_shapes(&L);
  const uint64_t nf = L.nf, n = nf + L.nc, k = (uint64_t)K;
  if (lev_has_comp(&L)) {
    int rc = 0;
    for (int j = 0; j < K && rc == 0; j++) {
      amgd_route_hit(AMGD_R_VC_MR_COMP);
      rc = amgd_vc_level_run(Af, W, AfP, D, m, rho, X + j * n, B + j * nf, C_out + j * nf, 1);
    }
    return rc;
  }
  L.beta = (double *)calloc(m + 1, 8);
  L.gamma = (double *)calloc(m + 1, 8);
  cheb_scalars(rho, m, L.beta, L.gamma);
  double *x = dalloc(n * k), *b = dalloc(nf * k), *c0 = dalloc(nf * k), *c1 = dalloc(nf * k);
  const amgd_cptr8 iX = amgd_cptr8_strided(X, n, K), iB = amgd_cptr8_strided(B, nf, K);
  const amgd_ptr8 oX = amgd_ptr8_strided(X, n, K), oB = amgd_ptr8_strided(B, nf, K), oC = amgd_ptr8_strided(C_out, nf, K);
  amgd_vcn_scatter(x, &iX, NULL, n, K);
  amgd_vcn_scatter(b, &iB, NULL, nf, K);
  g_mr_fam_run = family;
  const double *c = vc_up_n(&L, K, x + nf * k, x, b, c0, c1);
  g_mr_fam_run = -1;
  amgd_vcn_gather(&oX, x, NULL, nf, K, 0, NULL);
  amgd_vcn_gather(&oB, b, NULL, nf, K, 0, NULL);
  amgd_vcn_gather(&oC, c, NULL, nf, K, 0, NULL);
  amgd_sync();
  amgd_free(x); amgd_free(b); amgd_free(c0); amgd_free(c1);
  free(L.beta); free(L.gamma);
  return 0;
}
/* BC (K columns of nc) += W' BF (K columns of nf) with W' = amgd_transpose(W) */
int amgd_vc_restrict_run_n(const dcsr *W, double *BF, double *BC, int K, int family) {
  if (K != 2 && K != 4 && K != 8) return -1;
  vc_lev L;
  memset(&L, 0, sizeof L);
  L.Wt = amgd_transpose(W, NULL);
  L.sh_r = mat_shape(L.Wt);
  const uint64_t nf = W->rn, nc = W->cn, k = (uint64_t)K;
  if (L.sh_r == VC_COMP) {
    for (int j = 0; j < K; j++) {
      amgd_route_hit(AMGD_R_VC_MR_COMP);
      vc_restrict(&L, BF + j * nf, BC + j * nc, 1);
    }
  } else {
    double *bf = dalloc(nf * k), *bc = dalloc(nc * k);
    const amgd_cptr8 iF = amgd_cptr8_strided(BF, nf, K), iC = amgd_cptr8_strided(BC, nc, K);
    const amgd_ptr8 oC = amgd_ptr8_strided(BC, nc, K);
    amgd_vcn_scatter(bf, &iF, NULL, nf, K);
    amgd_vcn_scatter(bc, &iC, NULL, nc, K);
    g_mr_fam_run = family;
    vc_restrict_n(&L, K, bf, bc);
    g_mr_fam_run = -1;
    amgd_vcn_gather(&oC, bc, NULL, nc, K, 0, NULL);
    amgd_sync();
    amgd_free(bf); amgd_free(bc);
  }
  amgd_sync();
  dcsr_free(&L.Wt);
  return 0;
}
