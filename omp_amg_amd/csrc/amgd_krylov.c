/*
 * amgd_krylov.c -- restarted flexible GMRES on the kept hierarchy, preconditioned from the
 * right by the V-cycle (host driver, C; kernels amgd_krylov.hip; DESIGN.md "Krylov" has the
 * contract).
 *
 * The cycle is not a symmetric operator (its restriction is b_C + W' b_F, its prolongation
 * W x_C + P(b_F - AfP x_C)), so the wrapper is GMRES, and flexible because nothing asks the
 * preconditioner to be the same linear map at every step.  Classical Gram-Schmidt applied
 * twice: all dots of a pass are taken against the same w, then w is updated by the whole
 * basis.  Two dot paths share every other kernel: ordered (every dot amgd_dot with the exact
 * left-to-right summation forced on, a host restatement reproduces the solve bit for bit) and
 * fused (one multi-dot sweep per pass, fixed-order partial sums, one host synchronisation per
 * inner iteration).  Compiled with -ffp-contract=off: the rotations and the back-substitution
 * round like the restatement's.
 *
 * The workspace -- V (m + 1 vectors), Z (m vectors), w, x, r, the small scalar block and the
 * multi-dot's partials -- is kept with the hierarchy beside the solve plan, regrown when m
 * grows and freed with the hierarchy.
 *
 * A row-partitioned hierarchy (flag bit 2; DESIGN.md "Krylov on the row-partitioned hierarchy")
 * is solved by the same loop on each rank's rows: the Krylov vectors hold the own rows, the
 * cycle is the partitioned cycle on own-row vectors, the level-0 product runs on the rank's row
 * block of A against a whole-length operand whose halo entries are fetched first, and a dot is
 * either both operands completed on every rank (ordered: bit for bit the one-GPU solve) or the
 * ranks' fused sums gathered and added in rank order by one kernel (k_kry_comb).
 *
 * Second half of the file: amgd_krylov_device_n, several right-hand sides of one operator solved
 * in lock-step on a slot per column (DESIGN.md "Krylov on several right-hand sides").  Both
 * drivers run the same per-column host arithmetic and the same launches (kry_host_*, kry_dev_*);
 * the lock-step cycles go through the V-cycle driver's own group loop (amgd_vc_cycles_n).
 */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "amgd.h"
#include "amgd_drv.h"
#include "omp_amg_amd.h"

#define API __attribute__((visibility("default")))
#define KRY_MAXB (AMGD_KRYLOV_MAX_RESTART + 1)
/* the scalar block (doubles): pass-1 dots, pass-2 dots, the Hessenberg column d + d' with the
   norm behind it, y of the back-substitution, ||w||^2, beta / a single dot */
enum { SC_C1 = 0, SC_C2 = 72, SC_HS = 144, SC_Y = 216, SC_NRM = 288, SC_ONE = 290, SC_N = 296 };

struct amgd_kry_ws {
  uint32_t m;                     /* basis size the blocks were made for */
  uint64_t n, ld;                 /* rows of a vector (partitioned: this rank's), the basis stride */
  double *V, *Z, *w, *x, *r, *sc, *part;
  /* a row-partitioned hierarchy (DESIGN.md "Krylov on the row-partitioned hierarchy"): the
     vectors above hold this rank's rows; zop is the whole-length operand of the level-0
     product (valid on the own rows and the halo entries only), gath the ranks' partial sums
     (np x KRY_MAXB), ga / gb the ordered path's whole-length operands (made when it first runs) */
  int ispart, np, me;
  uint32_t r0;
  uint64_t n0;
  const uint64_t *rowoff;         /* the plan's: byte offsets of the level-0 rows by rank */
  amgd_hier *h;
  double *zop, *gath, *ga, *gb;
};

void amgd_kry_ws_free_host(struct amgd_kry_ws **wp) {
  free(*wp);
  *wp = NULL;
}
void amgd_kry_ws_free(struct amgd_kry_ws **wp) {
  struct amgd_kry_ws *w = *wp;
  if (!w) return;
  double *blk[11] = {w->V, w->Z, w->w, w->x, w->r, w->sc, w->part, w->zop, w->gath, w->ga, w->gb};
  for (int k = 0; k < 11; k++) if (blk[k]) amgd_free(blk[k]);
  amgd_kry_ws_free_host(wp);
}
static int ws_body(void *arg) {
  struct amgd_kry_ws *w = (struct amgd_kry_ws *)arg;
  w->V = dalloc((uint64_t)(w->m + 1) * w->ld);
  w->Z = dalloc((uint64_t)w->m * w->ld);
  w->w = dalloc(w->n); w->x = dalloc(w->n); w->r = dalloc(w->n);
  w->sc = dalloc(SC_N);
  w->part = dalloc((uint64_t)KRY_MAXB * (uint64_t)amgd_kry_grid(w->n));
  if (w->ispart) {
    w->zop = dalloc(w->n0);
    w->gath = dalloc((uint64_t)w->np * KRY_MAXB);
  }
  return 0;
}
static int ws_ordered_body(void *arg) {
  struct amgd_kry_ws *w = (struct amgd_kry_ws *)arg;
  w->ga = dalloc(w->n0);
  w->gb = dalloc(w->n0);
  return 0;
}
/* the V-cycle driver's side of a partitioned plan (amgd_vcycle.c) */
void amgd_vc_part_info(const amgd_hier *h, int *np, int *me, uint32_t *r0, uint32_t *r1, const uint64_t **rowoff);
int amgd_vc_a0_has_exchange(const amgd_hier *h);
int amgd_vc_a0_exchange(amgd_hier *h, double *v, uint64_t *bytes);
int amgd_vc_solve_own(amgd_hier *h, double *xo, const double *bo, int flags);
/* the workspace for basis size m; the plan exists.  ordered: a partitioned hierarchy's ordered
   path needs its two whole-length operands */
static int ws_ensure(amgd_hier *h, uint32_t m, int ordered) {
  int np = 1, me = 0;
  uint32_t r0 = 0, r1 = h->n0;
  const uint64_t *rowoff = NULL;
  if (h->part) amgd_vc_part_info(h, &np, &me, &r0, &r1, &rowoff);
  struct amgd_kry_ws *w = h->kry;
  if (!(w && w->m >= m && w->n == (uint64_t)(r1 - r0) && w->n0 == h->n0 && w->np == np && w->r0 == r0)) {
    amgd_kry_ws_free(&h->kry);
    w = (struct amgd_kry_ws *)calloc(1, sizeof *w);
    w->m = m;
    w->n = r1 - r0;
    w->n0 = h->n0;
    w->ld = (w->n + 1) & ~(uint64_t)1;      /* even: every column 16-byte aligned */
    w->ispart = h->part; w->np = np; w->me = me; w->r0 = r0;
    if (amgd_try(ws_body, w) != 0) { free(w); return -2; }   /* the blocks: released by the unwind */
    h->kry = w;
  }
  w->h = h;
  w->rowoff = rowoff;                       /* the plan may have been rebuilt since */
  if (w->ispart && ordered && !w->ga) {
    if (amgd_try(ws_ordered_body, w) != 0) { w->ga = w->gb = NULL; return -2; }
  }
  return 0;
}

static uint64_t g_calls, g_its;
/* collectives and bytes all ranks send in the call running, the cycles' included */
static uint64_t g_kc_coll, g_kc_bytes;
API void amgd_krylov_comm_stats(uint64_t *collectives, uint64_t *bytes) {
  if (collectives) *collectives = g_kc_coll;
  if (bytes) *bytes = g_kc_bytes;
}

typedef struct {
  amgd_hier *h;
  double *dx;
  const double *db;
  amgd_krylov_opts o;
  amgd_krylov_info *info;
  double *hist;
  uint32_t hist_cap;
} kry_args;

/* ---- several ranks: the Krylov vectors hold a rank's own rows ---- */
static uint64_t *g_goff;          /* host, np + 1: byte offsets of the ranks' sums for the nb in hand */
/* the ranks' nb partial sums, rank r's at gath + r*nb, completed on every rank and added in
   rank order: out[t] = (p_0[t] + p_1[t]) + ...; prev / hsum / root as k_kry_fin applies them */
static void kry_combine(const struct amgd_kry_ws *W, int nb, double *out, const double *prev, double *hsum,
                        double *root) {
  for (int r = 0; r <= W->np; r++) g_goff[r] = 8ull * (uint64_t)r * (uint64_t)nb;
  void *buf = W->gath;
  amgd_allgatherv(1, &buf, g_goff);
  g_kc_coll++;
  g_kc_bytes += 8ull * (uint64_t)nb * (uint64_t)W->np * (uint64_t)(W->np - 1);
  amgd_kry_comb(W->gath, W->np, nb, out, prev, hsum, root);
  amgd_route_hit(AMGD_R_KRY_P_COMB);
}
/* the multi-dot of a pass on the own rows, combined across the ranks (one rank: the one-GPU launches) */
static void kry_mdot_ranks(const struct amgd_kry_ws *W, const double *V, uint64_t ld, const double *w, int nb,
                           double *d, const double *prev, double *hsum) {
  if (W->np <= 1) { amgd_kry_mdot(V, ld, w, W->n, nb, W->part, d, prev, hsum); return; }
  amgd_kry_mdot(V, ld, w, W->n, nb, W->part, W->gath + (uint64_t)W->me * (uint64_t)nb, NULL, NULL);
  kry_combine(W, nb, d, prev, hsum, NULL);
}
/* the update that leaves ||w||^2 and its root, the partials combined the same way */
static void kry_axpys_norm_ranks(const struct amgd_kry_ws *W, double *w, const double *V, uint64_t ld, const double *c,
                                 int nb, double *nrm2, double *root) {
  if (W->np <= 1) { amgd_kry_axpys(w, V, ld, c, nb, W->n, 0, W->part, nrm2, root); return; }
  amgd_kry_axpys(w, V, ld, c, nb, W->n, 0, W->part, W->gath + W->me, W->sc + SC_ONE + 1);
  kry_combine(W, 1, nrm2, NULL, NULL, root);
}
/* whole (n0) from the ranks' own rows */
static void kry_gather(const struct amgd_kry_ws *W, double *whole, const double *own) {
  amgd_d2d(whole + W->r0, own, W->n * 8);
  if (W->np <= 1) return;
  void *buf = whole;
  amgd_allgatherv(1, &buf, W->rowoff);
  g_kc_coll++;
  g_kc_bytes += 8ull * W->n0 * (uint64_t)(W->np - 1);
}
/* a . b: ordered, amgd_dot (exact summation is on for the call); fused, the multi-dot on one
   vector.  Partitioned, ordered: both operands completed on every rank, the dot taken by each;
   b_whole: b is the whole vector in W->ga already (a Gram-Schmidt pass gathers w once) */
static double kdot_w(const struct amgd_kry_ws *W, int ordered, const double *a, const double *b, int b_whole) {
  if (ordered) {
    amgd_route_hit(AMGD_R_KRY_ODOT);
    if (!W->ispart) return amgd_dot(a, b, W->n);
    if (!b) {                                      /* a . a */
      if (!b_whole) kry_gather(W, W->ga, a);
      return amgd_dot(W->ga, NULL, W->n0);
    }
    kry_gather(W, W->gb, a);
    if (!b_whole) kry_gather(W, W->ga, b);
    return amgd_dot(W->gb, W->ga, W->n0);
  }
  double s;
  kry_mdot_ranks(W, a, W->n, b, 1, W->sc + SC_ONE, NULL, NULL);
  amgd_d2h(&s, W->sc + SC_ONE, 8);
  return s;
}
static double kdot(const struct amgd_kry_ws *W, int ordered, const double *a, const double *b) {
  return kdot_w(W, ordered, a, b, 0);
}
/* the level-0 product, the setup's event timers off as inside a cycle (amgd_vcycle.c) */
static void kspmv(const dcsr *A, const double *x, double *z, double alpha, const double *y, double beta) {
  amgd_timers_enable(0);
  amgd_spmv(A, x, z, alpha, y, beta, NULL);
  amgd_timers_enable(1);
}
/* z = alpha*y + beta*(A x) on the workspace's rows.  Partitioned: A is the rank's row block
   with global columns, x goes into the whole-length operand, whose entries of other ranks
   that the rows read are fetched first (the plan's halo list, or one allgatherv) */
static void kprod(const struct amgd_kry_ws *W, const dcsr *A, const double *x, double *z, double alpha,
                  const double *y, double beta) {
  /* one rank owns every row: x is the whole operand already (the copy below measured 11.9 us
     per product at 128^3) */
  if (W->np <= 1) { kspmv(A, x, z, alpha, y, beta); return; }
  amgd_d2d(W->zop + W->r0, x, W->n * 8);
  if (amgd_vc_a0_has_exchange(W->h)) {
    g_kc_coll += (uint64_t)amgd_vc_a0_exchange(W->h, W->zop, &g_kc_bytes);
    amgd_route_hit(AMGD_R_KRY_P_XCH);
  }
  if (W->n) kspmv(A, W->zop, z, alpha, y, beta);
}
static int finite_all(const double *v, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) if (!isfinite(v[i])) return 0;
  return 1;
}

/* ------------------------------------------------------------------------ */
/* One column of the solve, in pieces: the host arithmetic (kry_host_*) and the launches that  */
/* are the same on every path (kry_dev_*).  amgd_krylov_device runs them in sequence on its    */
/* one workspace; amgd_krylov_device_n runs them on a slot per column in lock-step.            */
/* ------------------------------------------------------------------------ */
/* H: column j at H + j*(m+1); c, s: the rotations; g: the rotated right-hand side */
typedef struct {
  double H[AMGD_KRYLOV_MAX_RESTART * KRY_MAXB], c[KRY_MAXB], s[KRY_MAXB], g[KRY_MAXB], y[KRY_MAXB];
  double target;
  uint32_t j, k;                  /* the inner index; columns of this restart */
} kry_host;
enum { KRY_DONE = 0, KRY_MAXIT = 1, KRY_GO = 2 };   /* a column's state: the first two are its rc */

/* x and r of the start: bnorm = ||b||, beta = ||r|| */
static void kry_dev_start(const struct amgd_kry_ws *W, const dcsr *A, const amgd_krylov_opts *o, const double *b,
                          const double *guess, double *bnorm, double *beta) {
  const int ordered = o->flags & 1;
  *bnorm = sqrt(kdot(W, ordered, b, b));
  if (o->flags & 2) {
    amgd_d2d(W->x, guess, W->n * 8);
    kprod(W, A, W->x, W->r, 1.0, b, -1.0);
    *beta = sqrt(kdot(W, ordered, W->r, W->r));
  } else {
    amgd_vfill(W->x, W->n, 0.0);
    amgd_d2d(W->r, b, W->n * 8);
    *beta = *bnorm;
  }
}
/* -4, KRY_DONE (converged at the start) or KRY_GO */
static int kry_host_start(kry_host *S, amgd_krylov_info *info, const amgd_krylov_opts *o, double bnorm, double beta) {
  if (!isfinite(bnorm) || !isfinite(beta)) return -4;
  const double rt = o->rtol * bnorm;
  S->target = rt > o->atol ? rt : o->atol;
  info->bnorm = bnorm;
  info->r0 = info->resid = beta;
  if (beta <= S->target) { info->converged = 1; return KRY_DONE; }
  return KRY_GO;
}
/* a restart begins: v_0 = r / beta */
static void kry_dev_restart(const struct amgd_kry_ws *W, kry_host *S, double beta) {
  amgd_h2d(W->sc + SC_ONE, &beta, 8);
  amgd_kry_scale(W->V, W->r, W->sc + SC_ONE, W->n);
  S->g[0] = beta;
  S->j = S->k = 0;
}
/* classical Gram-Schmidt twice on w against v_0 .. v_j with ordered dots, v_{j+1} = w / h_{j+1}:
   col[0 .. j] = d + d', returns h_{j+1} */
static double kry_dev_gs_ordered(const struct amgd_kry_ws *W, uint32_t j, double *col) {
  const uint64_t n = W->n, ld = W->ld;
  const int nb = (int)j + 1;
  double *w = W->w, *sc = W->sc, *vj = W->V + (uint64_t)j * ld;
  double d1[KRY_MAXB] = {0}, d2[KRY_MAXB] = {0};
  if (W->ispart) kry_gather(W, W->ga, w);                /* w once per pass, each v_i once per dot */
  for (int i = 0; i < nb; i++) d1[i] = kdot_w(W, 1, W->V + (uint64_t)i * ld, w, 1);
  amgd_h2d(sc + SC_C1, d1, (size_t)nb * 8);
  amgd_kry_axpys(w, W->V, ld, sc + SC_C1, nb, n, 0, W->part, NULL, NULL);
  if (W->ispart) kry_gather(W, W->ga, w);
  for (int i = 0; i < nb; i++) d2[i] = kdot_w(W, 1, W->V + (uint64_t)i * ld, w, 1);
  amgd_h2d(sc + SC_C2, d2, (size_t)nb * 8);
  amgd_kry_axpys(w, W->V, ld, sc + SC_C2, nb, n, 0, W->part, NULL, NULL);
  for (int i = 0; i < nb; i++) col[i] = d1[i] + d2[i];
  const double hn = sqrt(kdot(W, 1, w, NULL));
  amgd_h2d(sc + SC_HS + nb, &hn, 8);
  amgd_kry_scale(vj + ld, w, sc + SC_HS + nb, n);        /* v_{j+1} = w / h_{j+1} */
  return hn;
}
/* iteration j's Hessenberg column col[0 .. j] with h_{j+1} = hn arrived: the earlier rotations
   on it, the rotation that clears h_{j+1}, the residual estimate.  -4 a non-finite entry, 1 the
   restart ends here, 0 it goes on (the caller advances j) */
static int kry_host_step(kry_host *S, double *col, double hn, uint32_t m, uint32_t maxit, amgd_krylov_info *info,
                         double *hist, uint32_t hist_cap) {
  const uint32_t j = S->j;
  double *c = S->c, *s = S->s, *g = S->g;
  col[j + 1] = hn;
  if (!finite_all(col, j + 2)) return -4;
  info->its++;
  amgd_route_hit(AMGD_R_KRY_IT);
  for (uint32_t i = 0; i < j; i++) {
    const double t = c[i] * col[i] + s[i] * col[i + 1];
    col[i + 1] = -s[i] * col[i] + c[i] * col[i + 1];
    col[i] = t;
  }
  const double d = sqrt(col[j] * col[j] + col[j + 1] * col[j + 1]);
  c[j] = col[j] / d;
  s[j] = col[j + 1] / d;
  col[j] = c[j] * col[j] + s[j] * col[j + 1];
  memcpy(S->H + (size_t)j * KRY_MAXB, col, ((size_t)j + 1) * 8);
  g[j + 1] = -s[j] * g[j];
  g[j] = c[j] * g[j];
  const double est = fabs(g[j + 1]);
  if (hist && info->its <= hist_cap) hist[info->its - 1] = est;
  S->k = j + 1;
  return est <= S->target || S->k == m || info->its == maxit || hn == 0.;
}
/* y from the triangle */
static void kry_host_solve(kry_host *S) {
  const uint32_t k = S->k;
  double *y = S->y;
  for (uint32_t i = k; i-- > 0;) {
    double t = S->g[i];
    for (uint32_t l = i + 1; l < k; l++) t = t - S->H[(size_t)l * KRY_MAXB + i] * y[l];
    y[i] = t / S->H[(size_t)i * KRY_MAXB + i];
  }
}
/* x = ((x + y_0 z_0) + y_1 z_1) + ... */
static void kry_dev_update(const struct amgd_kry_ws *W, const kry_host *S) {
  amgd_h2d(W->sc + SC_Y, S->y, (size_t)S->k * 8);
  amgd_kry_axpys(W->x, W->Z, W->ld, W->sc + SC_Y, (int)S->k, W->n, 1, W->part, NULL, NULL);
}
/* beta: the true residual's norm after a restart.  -4, KRY_DONE, KRY_MAXIT or KRY_GO (another restart) */
static int kry_host_restart(amgd_krylov_info *info, double beta, double target, uint32_t maxit) {
  if (!isfinite(beta)) return -4;
  info->resid = beta;
  if (beta <= target) { info->converged = 1; return KRY_DONE; }
  if (info->its >= maxit) return KRY_MAXIT;
  info->restarts++;
  return KRY_GO;
}

static int kry_body(void *arg) {
  kry_args *a = (kry_args *)arg;
  amgd_hier *h = a->h;
  const struct amgd_kry_ws *W = h->kry;
  /* partitioned: the rank's row block of A, and of db and dx its own rows */
  const dcsr *A = h->part ? h->lv[0].A.p->m : h->lv[0].A.d;
  const uint64_t n = W->n, ld = W->ld;
  const uint32_t m = a->o.restart, maxit = a->o.maxit;
  const int ordered = a->o.flags & 1, cyc_flags = h->nullspace ? 1 : 0;
  const double *b = a->db + W->r0;
  double *xout = a->dx + W->r0;
  amgd_krylov_info *info = a->info;
  double *w = W->w, *sc = W->sc;
  kry_host S;
  double col[KRY_MAXB + 1];

  memset(info, 0, sizeof *info);
  double bnorm, beta;
  kry_dev_start(W, A, &a->o, b, xout, &bnorm, &beta);
  int st = kry_host_start(&S, info, &a->o, bnorm, beta);
  if (st < 0) return st;
  while (st == KRY_GO) {
    kry_dev_restart(W, &S, beta);
    for (;; S.j++) {
      const uint32_t j = S.j;
      double *vj = W->V + (uint64_t)j * ld, *zj = W->Z + (uint64_t)j * ld;
      const int nb = (int)j + 1;
      const int rc = h->part ? amgd_vc_solve_own(h, zj, vj, cyc_flags) : amgd_solve_device(h, zj, vj, cyc_flags);  /* z_j = cycle(v_j) */
      if (rc != 0) return rc;
      info->cycles++;
      if (h->part) {
        uint64_t cc, cb;
        amgd_solve_comm_stats(&cc, &cb);
        g_kc_coll += cc;
        g_kc_bytes += cb;
      }
      kprod(W, A, zj, w, 0.0, NULL, 1.0);                      /* w = A z_j */
      double hn;
      if (ordered) {
        hn = kry_dev_gs_ordered(W, j, col);
      } else {
        /* nothing here waits for the host: the update reads the dots from device memory, the
           last pass leaves d + d' with the norm behind it, and one download fetches them */
        kry_mdot_ranks(W, W->V, ld, w, nb, sc + SC_C1, NULL, NULL);
        amgd_kry_axpys(w, W->V, ld, sc + SC_C1, nb, n, 0, W->part, NULL, NULL);
        kry_mdot_ranks(W, W->V, ld, w, nb, sc + SC_C2, sc + SC_C1, sc + SC_HS);
        kry_axpys_norm_ranks(W, w, W->V, ld, sc + SC_C2, nb, sc + SC_NRM, sc + SC_HS + nb);
        amgd_kry_scale(vj + ld, w, sc + SC_HS + nb, n);
        amgd_d2h(col, sc + SC_HS, (size_t)(nb + 1) * 8);
        hn = col[nb];
      }
      st = kry_host_step(&S, col, hn, m, maxit, info, a->hist, a->hist_cap);
      if (st < 0) return st;
      if (st) break;
    }
    kry_host_solve(&S);
    kry_dev_update(W, &S);
    kprod(W, A, W->x, W->r, 1.0, b, -1.0);                     /* the true residual */
    beta = sqrt(kdot(W, ordered, W->r, W->r));
    st = kry_host_restart(info, beta, S.target, maxit);
    if (st < 0) return st;
  }
  amgd_d2d(xout, W->x, n * 8);
  if (h->part && (a->o.flags & 8) && W->np > 1) {              /* dx whole on every rank */
    void *buf = a->dx;
    amgd_allgatherv(1, &buf, W->rowoff);
    g_kc_coll++;
    g_kc_bytes += 8ull * W->n0 * (uint64_t)(W->np - 1);
  }
  return info->converged ? 0 : 1;
}

API int amgd_krylov_device(amgd_hier *h, double *dx, const double *db, const amgd_krylov_opts *o,
                           amgd_krylov_info *info, double *hist, uint32_t hist_cap) {
  if (!h || !dx || !db || !o || !info || h->nlevels == 0 || h->n0 == 0) return -1;
  if (o->restart > AMGD_KRYLOV_MAX_RESTART || !(o->rtol >= 0) || !(o->atol >= 0)) return -1;
  /* the partitioned call is collective and works on a rank's own rows: a caller says so with
     flag bit 2, as for amgd_solve_device; without it a partitioned hierarchy is refused */
  if (h->part && !(o->flags & 4)) return -3;
  kry_args a = {h, dx, db, *o, info, hist, hist_cap};
  if (!a.o.restart) a.o.restart = 30;
  if (!a.o.maxit) a.o.maxit = 100;
  g_kc_coll = g_kc_bytes = 0;
  /* a partitioned hierarchy is solved in partitioned mode whatever the communicator's flag says now */
  const int was = amgd_comm_part_get();
  if (h->part) amgd_comm_part_set(1);
  /* the plan, then the workspace, then the iteration: each in an amgd_try of its own, so an
     unwind releases what its step allocated and nothing an earlier step keeps */
  int rc = amgd_vc_prepare(h);
  if (rc == 0 && ws_ensure(h, a.o.restart, a.o.flags & 1) != 0) rc = -2;
  if (rc == 0 && h->part && h->kry->np > 1) {
    free(g_goff);
    g_goff = (uint64_t *)malloc(((size_t)h->kry->np + 1) * 8);
    if (!g_goff) rc = -2;
  }
  if (rc != 0) { amgd_comm_part_set(was); return rc; }
  const int ex = amgd_get_exact();
  if (a.o.flags & 1) amgd_set_exact(1);
  amgd_xtimer_begin(AMGD_XT_KRY);
  rc = amgd_try(kry_body, &a);
  amgd_timers_enable(1);
  amgd_xtimer_end(AMGD_XT_KRY);
  amgd_set_exact(ex);
  amgd_comm_part_set(was);
  g_calls++;
  g_its += info->its;
  if (rc < 0) amgd_sync();
  return rc;
}

API void amgd_krylov_stats(uint64_t *calls, uint64_t *its, double *ms) {
  if (calls) *calls = g_calls;
  if (its) *its = g_its;
  if (ms) *ms = amgd_xtimer_ms(AMGD_XT_KRY);
}

/* the combined multi-dot and the combined norm of an update on their own (amgd_testapi.c): the
   solver's own launches on a rank's rows V (nb columns of stride ld), w and c (device); every
   rank of the partitioned communicator calls.  d: nb sums; nrm: ||w||^2 and its root */
static void ranks_ws(struct amgd_kry_ws *W, uint64_t n, int nb) {
  memset(W, 0, sizeof *W);
  W->np = amgd_pcomm_size();
  W->me = amgd_pcomm_rank();
  W->n = n;
  W->part = dalloc((uint64_t)nb * (uint64_t)amgd_kry_grid(n));
  W->gath = dalloc((uint64_t)W->np * KRY_MAXB);
  W->sc = dalloc(SC_N);
  free(g_goff);
  g_goff = (uint64_t *)malloc(((size_t)W->np + 1) * 8);
}
static void ranks_ws_free(struct amgd_kry_ws *W) {
  amgd_sync();
  amgd_free(W->part); amgd_free(W->gath); amgd_free(W->sc);
}
void amgd_kry_mdot_ranks_run(const double *V, uint64_t ld, const double *w, uint64_t n, int nb, double *d) {
  struct amgd_kry_ws W;
  ranks_ws(&W, n, nb);
  kry_mdot_ranks(&W, V, ld, w, nb, d, NULL, NULL);
  ranks_ws_free(&W);
}
void amgd_kry_norm_ranks_run(double *w, const double *V, uint64_t ld, const double *c, int nb, uint64_t n, double *nrm) {
  struct amgd_kry_ws W;
  ranks_ws(&W, n, nb);
  kry_axpys_norm_ranks(&W, w, V, ld, c, nb, nrm, nrm + 1);
  ranks_ws_free(&W);
}

/* one cycle and one level-0 product, timed like a solve (amgd_testapi.c): what an inner
   iteration costs before any orthogonalisation */
int amgd_kry_floor(amgd_hier *h, double *dx, const double *db) {
  if (!h || h->part || !h->kry || !dx || !db) return -1;
  amgd_xtimer_begin(AMGD_XT_KRY);
  const int rc = amgd_solve_device(h, dx, db, h->nullspace ? 1 : 0);
  if (rc == 0) kspmv(h->lv[0].A.d, dx, h->kry->w, 0.0, NULL, 1.0);
  amgd_xtimer_end(AMGD_XT_KRY);
  return rc;
}

/* ------------------------------------------------------------------------ */
/* several right-hand sides in lock-step (DESIGN.md "Krylov on several right-hand sides")      */
/* ------------------------------------------------------------------------ */
/* nrhs independent solves share S slots.  A slot owns what amgd_krylov_device's workspace
   holds -- V, Z, w, x, r, a scalar block, multi-dot partials -- and the host state of the
   column it serves.  The columns are taken in ascending order; when a slot's column finishes,
   the next pending column takes the slot at the next step, so the groups stay full and the
   active columns ordinarily stand at different j.  One step serves every active slot at its
   own j: the cycles through the V-cycle driver's group loop (amgd_vc_cycles_n, the one
   amgd_solve_device_n runs), the level-0 products through the K-column product
   (amgd_krylov_mrhs.hip), both in groups of 8 / 4 / 2 formed greedily under the AMGD_VC_MRHS_K
   mask (amgd_vc_group_size; a leftover takes the single-vector form), the two
   Gram-Schmidt passes of all columns in single launches with ONE download, then each column's
   host arithmetic -- the functions above, the single solver's own.  Column j comes out bit for
   bit as amgd_krylov_device gives it: every kernel a column passes through keeps that column's
   operation order whatever runs beside it.
   The slots' vectors are one block of S (2 m + 4) vectors of even ld, S (2 m + 4) n0 8 B: at
   m = 30 and S = 8, 68.7 GB at 256^3 (n0 = 16.8 M) -- a caller short of HBM lowers AMGD_KRY_SLOTS
   or the restart length.  Kept on the hierarchy, regrown when S or m grows, freed with it. */
#define KRY_SLOTS_MAX 8
#define KRY_SLOTS_DEFAULT 8
typedef struct {
  struct amgd_kry_ws W;           /* this slot's part of the shared blocks */
  kry_host S;
  int col;                        /* the column served, -1: idle */
  int fresh;                      /* the next step begins a restart */
  double beta;
} kry_slot;
struct amgd_kry_nws {
  uint32_t S, m;
  uint64_t n, ld;
  double *vec, *sc, *part;
  kry_slot slot[KRY_SLOTS_MAX];
  double hs[KRY_SLOTS_MAX * SC_N];   /* host: the step's download */
};
void amgd_kry_nws_free_host(struct amgd_kry_nws **wp) {
  free(*wp);
  *wp = NULL;
}
void amgd_kry_nws_free(struct amgd_kry_nws **wp) {
  struct amgd_kry_nws *w = *wp;
  if (!w) return;
  if (w->vec) amgd_free(w->vec);
  if (w->sc) amgd_free(w->sc);
  if (w->part) amgd_free(w->part);
  amgd_kry_nws_free_host(wp);
}
static int nws_body(void *arg) {
  struct amgd_kry_nws *w = (struct amgd_kry_nws *)arg;
  w->vec = dalloc((uint64_t)w->S * (2ull * w->m + 4) * w->ld);
  w->sc = dalloc((uint64_t)w->S * SC_N);
  w->part = dalloc((uint64_t)w->S * KRY_MAXB * (uint64_t)amgd_kry_grid(w->n));
  return 0;
}
static int nws_ensure(amgd_hier *h, uint32_t S, uint32_t m) {
  if (h->kryn && h->kryn->S >= S && h->kryn->m >= m && h->kryn->n == h->n0) return 0;
  if (h->kryn) {                                  /* regrown: never smaller in either */
    if (h->kryn->n == h->n0) { if (h->kryn->S > S) S = h->kryn->S; if (h->kryn->m > m) m = h->kryn->m; }
    amgd_kry_nws_free(&h->kryn);
  }
  struct amgd_kry_nws *w = (struct amgd_kry_nws *)calloc(1, sizeof *w);
  if (!w) return -2;
  w->S = S;
  w->m = m;
  w->n = h->n0;
  w->ld = (w->n + 1) & ~(uint64_t)1;      /* even: every vector 16-byte aligned */
  if (amgd_try(nws_body, w) != 0) { free(w); return -2; }   /* the blocks: released by the unwind */
  const uint64_t G = (uint64_t)amgd_kry_grid(w->n);
  for (uint32_t s = 0; s < S; s++) {
    struct amgd_kry_ws *W = &w->slot[s].W;
    W->m = m;
    W->n = w->n;
    W->ld = w->ld;
    W->V = w->vec + (uint64_t)s * (2ull * m + 4) * w->ld;
    W->Z = W->V + (uint64_t)(m + 1) * w->ld;
    W->w = W->Z + (uint64_t)m * w->ld;
    W->x = W->w + w->ld;
    W->r = W->x + w->ld;
    W->sc = w->sc + (uint64_t)s * SC_N;
    W->part = w->part + (uint64_t)s * KRY_MAXB * G;
    w->slot[s].col = -1;
  }
  h->kryn = w;
  return 0;
}

/* the V-cycle driver's side (amgd_vcycle.c): the group sizes allowed and the next group's, the
   interleaved work vectors, the cycles of nc columns given by pointer, a matrix's row shape */
int amgd_vc_mrhs_mask(void);
int amgd_vc_group_size(int mask, int left);
int amgd_vc_mrhs_reserve(amgd_hier *h, int K);
double *amgd_vc_mrhs_scratch(const amgd_hier *h);
int amgd_vc_cycles_n(amgd_hier *h, int nc, const double *const *in, double *const *out, int flags, int single,
                     uint64_t *bytes);
int amgd_vc_mat_shape(const dcsr *M);

/* slots: kry_slots, 1..KRY_SLOTS_MAX (less than 1: the default).  The product's kernel family,
   kry_family: 0 by the mean row length (long rows from 16 entries on, the threshold of every
   other product here), 1 short-row, 2 long-row */
static int kry_slots(void) {
  const int64_t s = amgd_knob(AMGD_K_KRY_SLOTS);
  return s < 1 ? KRY_SLOTS_DEFAULT : s > KRY_SLOTS_MAX ? KRY_SLOTS_MAX : (int)s;
}
static int g_fam_run = -1;                 /* amgd_kry_products_run names its own for one call */
static int kry_family(void) {
  const int64_t f = g_fam_run >= 0 ? g_fam_run : amgd_knob(AMGD_K_KRY_FAMILY);
  return f < 0 || f > 2 ? 0 : (int)f;
}
/* z_q = alpha*y_q + beta*(A x_q) for nc columns (y NULL: none): K-column products in greedy
   groups, the leftover and every column of an outlier-row matrix through amgd_spmv */
static void products_n(const dcsr *A, double *scratch, int shape, int mask, int nc, const double *const *x,
                       double *const *z, double alpha, const double *const *y, double beta) {
  const int f = kry_family(), fam = f == 1 ? 0 : f == 2 ? 1 : shape == 2;
  for (int q = 0; q < nc;) {
    const int K = shape == 0 ? 0 : amgd_vc_group_size(mask, nc - q);
    if (!K) {
      amgd_route_hit(shape == 0 ? AMGD_R_KRY_N_COMP : AMGD_R_KRY_N_SINGLE);
      kspmv(A, x[q], z[q], alpha, y ? y[q] : NULL, beta);
      q++;
      continue;
    }
    const amgd_cptr8 X = amgd_cptr8_of(x + q, K), Y = amgd_cptr8_of(y ? y + q : NULL, y ? K : 0);
    const amgd_ptr8 Z = amgd_ptr8_of(z + q, K);
    amgd_route_hit(AMGD_R_KRY_N_PROD);
    amgd_kry_spmv_n(A, K, fam, &X, &Z, alpha, y ? &Y : NULL, beta, scratch);
    q += K;
  }
}
/* the product of one group of K columns on given device operands (amgd_testapi.c), routed as
   the solver routes it; family as the switch kry_family (negative: the switch itself) */
void amgd_kry_products_run(const dcsr *A, int K, int family, const double *const *x, double *const *z, double alpha,
                           const double *const *y, double beta) {
  double *scratch = dalloc((uint64_t)A->cn * (uint64_t)K);
  g_fam_run = family;
  products_n(A, scratch, amgd_vc_mat_shape(A), K, K, x, z, alpha, y, beta);
  g_fam_run = -1;
  amgd_sync();
  amgd_free(scratch);
}
#define KRY_PENDING (-1000)                /* rcs of a column that has not finished */
typedef struct {
  amgd_hier *h;
  double *dX;
  const double *dB;
  int nrhs;
  uint64_t ld;
  amgd_krylov_opts o;
  amgd_krylov_info *info;
  int *rcs;
  double *hist;
  uint32_t hist_cap;
  int S, next;                    /* slots in use; the next pending column */
  uint64_t steps;
} kryn_args;
static void col_finish(kryn_args *a, kry_slot *sl, int rc) {
  if (rc >= 0) amgd_d2d(a->dX + (uint64_t)sl->col * a->ld, sl->W.x, sl->W.n * 8);
  a->rcs[sl->col] = rc;
  sl->col = -1;
}
/* column c enters slot sl; it may finish at once (converged at the start, or -4) */
static void col_begin(kryn_args *a, kry_slot *sl, int c) {
  amgd_krylov_info *info = &a->info[c];
  const double *b = a->dB + (uint64_t)c * a->ld;
  memset(info, 0, sizeof *info);
  double bnorm, beta;
  kry_dev_start(&sl->W, a->h->lv[0].A.d, &a->o, b, a->dX + (uint64_t)c * a->ld, &bnorm, &beta);
  const int st = kry_host_start(&sl->S, info, &a->o, bnorm, beta);
  sl->col = c;
  if (st != KRY_GO) { col_finish(a, sl, st); return; }
  sl->fresh = 1;
  sl->beta = beta;
}
static int kryn_body(void *arg) {
  kryn_args *a = (kryn_args *)arg;
  amgd_hier *h = a->h;
  struct amgd_kry_nws *N = h->kryn;
  const uint64_t n = N->n, ld = N->ld;
  const uint32_t m = a->o.restart, maxit = a->o.maxit;
  const int ordered = a->o.flags & 1, cyc_flags = h->nullspace ? 1 : 0;
  const dcsr *A0 = h->lv[0].A.d;
  const int mask = amgd_vc_mrhs_mask(), shape = amgd_vc_mat_shape(A0);
  double *hs = N->hs;
  for (;;) {
    /* refill: every idle slot takes the next pending column */
    kry_slot *act[KRY_SLOTS_MAX];
    int na = 0;
    for (int s = 0; s < a->S; s++) {
      kry_slot *sl = &N->slot[s];
      while (sl->col < 0 && a->next < a->nrhs) col_begin(a, sl, a->next++);
      if (sl->col >= 0) act[na++] = sl;
    }
    if (!na) break;
    a->steps++;
    amgd_route_hit(AMGD_R_KRY_N_STEP);
    const double *vj[KRY_SLOTS_MAX];
    double *zj[KRY_SLOTS_MAX], *wq[KRY_SLOTS_MAX];
    int mixed = 0;
    for (int q = 0; q < na; q++) {
      kry_slot *sl = act[q];
      if (sl->fresh) { kry_dev_restart(&sl->W, &sl->S, sl->beta); sl->fresh = 0; }
      vj[q] = sl->W.V + (uint64_t)sl->S.j * ld;
      zj[q] = sl->W.Z + (uint64_t)sl->S.j * ld;
      wq[q] = sl->W.w;
      if (sl->S.j != act[0]->S.j) mixed = 1;
    }
    if (mixed) amgd_route_hit(AMGD_R_KRY_N_MIXED);
    const int rc = amgd_vc_cycles_n(h, na, vj, zj, cyc_flags, AMGD_R_KRY_N_SINGLE, NULL);   /* z_j = cycle(v_j) */
    if (rc != 0) return rc;
    for (int q = 0; q < na; q++) a->info[act[q]->col].cycles++;
    products_n(A0, amgd_vc_mrhs_scratch(h), shape, mask, na, (const double *const *)zj, wq, 0.0, NULL, 1.0);   /* w = A z_j */
    double hn[KRY_SLOTS_MAX], *col[KRY_SLOTS_MAX], ocol[KRY_SLOTS_MAX][KRY_MAXB + 1];
    if (ordered) {
      for (int q = 0; q < na; q++) {
        col[q] = ocol[q];
        hn[q] = kry_dev_gs_ordered(&act[q]->W, act[q]->S.j, col[q]);
      }
    } else {
      /* the single solver's five launches, each serving every active column; nothing waits for
         the host before the one download of the scalar blocks from the first active slot's
         Hessenberg column to the last one's */
      amgd_kry_col C[KRY_SLOTS_MAX];
      memset(C, 0, sizeof C);
      for (int q = 0; q < na; q++) {
        const struct amgd_kry_ws *W = &act[q]->W;
        C[q].V = W->V; C[q].w = W->w; C[q].nb = (int)act[q]->S.j + 1; C[q].part = W->part;
        C[q].d = W->sc + SC_C1;
      }
      amgd_kry_mdot_n(C, na, ld, n);
      amgd_kry_axpys_n(C, na, ld, n);
      for (int q = 0; q < na; q++) {
        double *sc = act[q]->W.sc;
        C[q].d = sc + SC_C2; C[q].prev = sc + SC_C1; C[q].hsum = sc + SC_HS;
      }
      amgd_kry_mdot_n(C, na, ld, n);
      for (int q = 0; q < na; q++) {
        double *sc = act[q]->W.sc;
        C[q].nrm2 = sc + SC_NRM; C[q].root = sc + SC_HS + C[q].nb;
        C[q].vout = act[q]->W.V + (uint64_t)C[q].nb * ld; C[q].h = C[q].root;
      }
      amgd_kry_axpys_n(C, na, ld, n);
      amgd_kry_scale_n(C, na, n);
      const double *lo = act[0]->W.sc + SC_HS, *hi = act[na - 1]->W.sc + SC_HS + C[na - 1].nb + 1;
      amgd_d2h(hs, lo, (size_t)(hi - lo) * 8);
      for (int q = 0; q < na; q++) {
        col[q] = hs + (act[q]->W.sc + SC_HS - lo);
        hn[q] = col[q][C[q].nb];
      }
    }
    /* each column's rotations and stopping test; the columns whose restart ends */
    kry_slot *end[KRY_SLOTS_MAX];
    int ne = 0;
    for (int q = 0; q < na; q++) {
      kry_slot *sl = act[q];
      const int c = sl->col;
      const int st = kry_host_step(&sl->S, col[q], hn[q], m, maxit, &a->info[c],
                                   a->hist ? a->hist + (uint64_t)c * a->hist_cap : NULL, a->hist_cap);
      if (st < 0) col_finish(a, sl, st);
      else if (st) end[ne++] = sl;
      else sl->S.j++;
    }
    if (!ne) continue;
    /* back-substitution, x += Z y, the true residuals r = b - A x in groups, their norms */
    const double *xq[KRY_SLOTS_MAX], *bq[KRY_SLOTS_MAX];
    double *rq[KRY_SLOTS_MAX], beta[KRY_SLOTS_MAX];
    for (int q = 0; q < ne; q++) {
      kry_slot *sl = end[q];
      kry_host_solve(&sl->S);
      kry_dev_update(&sl->W, &sl->S);
      xq[q] = sl->W.x;
      rq[q] = sl->W.r;
      bq[q] = a->dB + (uint64_t)sl->col * a->ld;
    }
    products_n(A0, amgd_vc_mrhs_scratch(h), shape, mask, ne, xq, rq, 1.0, bq, -1.0);
    if (ordered) {
      for (int q = 0; q < ne; q++) beta[q] = sqrt(kdot(&end[q]->W, 1, rq[q], rq[q]));
    } else {                               /* the launches first: the first download waits for all */
      for (int q = 0; q < ne; q++) {
        const struct amgd_kry_ws *W = &end[q]->W;
        amgd_kry_mdot(rq[q], n, rq[q], n, 1, W->part, W->sc + SC_ONE, NULL, NULL);
      }
      for (int q = 0; q < ne; q++) {
        amgd_d2h(&beta[q], end[q]->W.sc + SC_ONE, 8);
        beta[q] = sqrt(beta[q]);
      }
    }
    for (int q = 0; q < ne; q++) {
      kry_slot *sl = end[q];
      const int st = kry_host_restart(&a->info[sl->col], beta[q], sl->S.target, maxit);
      if (st != KRY_GO) { col_finish(a, sl, st); continue; }
      sl->fresh = 1;
      sl->beta = beta[q];
    }
  }
  return 0;
}

static uint64_t g_n_calls, g_n_cols, g_n_steps;
API int amgd_krylov_device_n(amgd_hier *h, double *dX, const double *dB, int nrhs, uint64_t ld,
                             const amgd_krylov_opts *o, amgd_krylov_info *info, int *rcs, double *hist,
                             uint32_t hist_cap) {
  if (!h || !dX || !dB || !o || !info || nrhs < 1 || h->nlevels == 0 || h->n0 == 0 || ld < h->n0) return -1;
  if (o->restart > AMGD_KRYLOV_MAX_RESTART || !(o->rtol >= 0) || !(o->atol >= 0)) return -1;
  if (h->part) return -3;
  int *own = (int *)malloc((size_t)nrhs * sizeof(int));
  if (!own) return -2;
  kryn_args a = {h, dX, dB, nrhs, ld, *o, info, own, hist, hist_cap, 0, 0, 0};
  if (!a.o.restart) a.o.restart = 30;
  if (!a.o.maxit) a.o.maxit = 100;
  a.S = kry_slots() < nrhs ? kry_slots() : nrhs;
  /* the plan with its interleaved work vectors, then the slots, then the iteration: each in an
     amgd_try of its own, so an unwind releases what its step allocated and nothing an earlier
     step keeps */
  int rc = amgd_vc_prepare(h);
  if (rc == 0) {
    const int K = amgd_vc_group_size(amgd_vc_mrhs_mask(), a.S);
    if (K && amgd_vc_mrhs_reserve(h, K) != 0) rc = -2;
  }
  if (rc == 0 && nws_ensure(h, (uint32_t)a.S, a.o.restart) != 0) rc = -2;
  if (rc != 0) { free(own); return rc; }
  for (int j = 0; j < nrhs; j++) own[j] = KRY_PENDING;
  for (int s = 0; s < KRY_SLOTS_MAX; s++) h->kryn->slot[s].col = -1;
  const int ex = amgd_get_exact();
  if (a.o.flags & 1) amgd_set_exact(1);
  amgd_xtimer_begin(AMGD_XT_KRYN);
  rc = amgd_try(kryn_body, &a);
  amgd_timers_enable(1);
  amgd_xtimer_end(AMGD_XT_KRYN);
  amgd_set_exact(ex);
  g_n_calls++;
  g_n_cols += (uint64_t)nrhs;
  g_n_steps += a.steps;
  if (rc != 0) amgd_sync();
  /* the call's value: the iteration's failure (the columns it left unfinished carry it), else
     -4 if any column is, else 1 if any column ran out of iterations */
  int worst = rc;
  for (int j = 0; j < nrhs; j++) {
    if (own[j] == KRY_PENDING) own[j] = rc != 0 ? rc : -2;
    if (rc == 0 && (own[j] == -4 || (own[j] == 1 && worst == 0))) worst = own[j];
    if (rcs) rcs[j] = own[j];
  }
  free(own);
  return worst;
}
API void amgd_krylov_n_stats(uint64_t *calls, uint64_t *columns, uint64_t *steps, double *ms) {
  if (calls) *calls = g_n_calls;
  if (columns) *columns = g_n_cols;
  if (steps) *steps = g_n_steps;
  if (ms) *ms = amgd_xtimer_ms(AMGD_XT_KRYN);
}

/* K cycles and K level-0 products in the groups a lock-step step forms, on the slots of an
   earlier amgd_krylov_device_n call of at least K columns, on that call's timer: what a step
   costs before any orthogonalisation (tools/solve_bench.py --krylov --nrhs) */
int amgd_kry_floor_n(amgd_hier *h, int K) {
  if (!h || h->part || !h->kryn || K < 1 || (uint32_t)K > h->kryn->S) return -1;
  const double *v[KRY_SLOTS_MAX];
  double *z[KRY_SLOTS_MAX], *w[KRY_SLOTS_MAX];
  for (int q = 0; q < K; q++) {
    v[q] = h->kryn->slot[q].W.V;
    z[q] = h->kryn->slot[q].W.Z;
    w[q] = h->kryn->slot[q].W.w;
  }
  const dcsr *A = h->lv[0].A.d;
  const int mask = amgd_vc_mrhs_mask();
  amgd_xtimer_begin(AMGD_XT_KRYN);
  const int rc = amgd_vc_cycles_n(h, K, v, z, h->nullspace ? 1 : 0, AMGD_R_KRY_N_SINGLE, NULL);
  if (rc == 0) products_n(A, amgd_vc_mrhs_scratch(h), amgd_vc_mat_shape(A), mask, K, (const double *const *)z, w, 0.0, NULL, 1.0);
  amgd_timers_enable(1);
  amgd_xtimer_end(AMGD_XT_KRYN);
  return rc;
}
