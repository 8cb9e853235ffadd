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
  uint64_t n, ld;
  double *V, *Z, *w, *x, *r, *sc, *part;
};

void amgd_kry_ws_free_host(struct amgd_kry_ws **wp) {
  free(*wp);
  *wp = NULL;
}
void amgd_kry_ws_free(struct amgd_kry_ws **wp) {
  struct amgd_kry_ws *w = *wp;
  if (!w) return;
  double *blk[7] = {w->V, w->Z, w->w, w->x, w->r, w->sc, w->part};
  for (int k = 0; k < 7; k++) if (blk[k]) amgd_free(blk[k]);
  amgd_kry_ws_free_host(wp);
}
static int ws_body(void *arg) {
  struct amgd_kry_ws *w = (struct amgd_kry_ws *)arg;
  w->V = dalloc((uint64_t)(w->m + 1) * w->ld);
  w->Z = dalloc((uint64_t)w->m * w->ld);
  w->w = dalloc(w->n); w->x = dalloc(w->n); w->r = dalloc(w->n);
  w->sc = dalloc(SC_N);
  w->part = dalloc((uint64_t)KRY_MAXB * (uint64_t)amgd_kry_grid(w->n));
  return 0;
}
static int ws_ensure(amgd_hier *h, uint32_t m) {
  if (h->kry && h->kry->m >= m && h->kry->n == h->n0) return 0;
  amgd_kry_ws_free(&h->kry);
  struct amgd_kry_ws *w = (struct amgd_kry_ws *)calloc(1, sizeof *w);
  w->m = m;
  w->n = h->n0;
  w->ld = (w->n + 1) & ~(uint64_t)1;      /* even: every column 16-byte aligned */
  if (amgd_try(ws_body, w) != 0) { free(w); return -2; }   /* the blocks: released by the unwind */
  h->kry = w;
  return 0;
}

void amgd_timers_enable(int on);
void amgd_kry_timer_begin(void);
void amgd_kry_timer_end(void);
double amgd_kry_timer_ms(void);
static uint64_t g_calls, g_its;
#define KRY_DRAIN 256

typedef struct {
  amgd_hier *h;
  double *dx;
  const double *db;
  amgd_krylov_opts o;
  amgd_krylov_info *info;
  double *hist;
  uint32_t hist_cap;
} kry_args;

/* a . b: ordered, amgd_dot (exact summation is on for the call); fused, the multi-dot on one vector */
static double kdot(const struct amgd_kry_ws *W, int ordered, const double *a, const double *b) {
  if (ordered) {
    amgd_route_hit(AMGD_R_KRY_ODOT);
    return amgd_dot(a, b, W->n);
  }
  double s;
  amgd_kry_mdot(a, W->n, b, W->n, 1, W->part, W->sc + SC_ONE, NULL, NULL);
  amgd_d2h(&s, W->sc + SC_ONE, 8);
  return s;
}
/* the level-0 product, the setup's event timers off as inside a cycle (amgd_vcycle.c) */
static void kspmv(const dcsr *A, const double *x, double *z, double alpha, const double *y, double beta) {
  amgd_timers_enable(0);
  amgd_spmv(A, x, z, alpha, y, beta, NULL);
  amgd_timers_enable(1);
}
static int finite_all(const double *v, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) if (!isfinite(v[i])) return 0;
  return 1;
}

static int kry_body(void *arg) {
  kry_args *a = (kry_args *)arg;
  amgd_hier *h = a->h;
  const struct amgd_kry_ws *W = h->kry;
  const dcsr *A = h->lv[0].A.d;
  const uint64_t n = W->n, ld = W->ld;
  const uint32_t m = a->o.restart, maxit = a->o.maxit;
  const int ordered = a->o.flags & 1, cyc_flags = h->nullspace ? 1 : 0;
  const double *b = a->db;
  amgd_krylov_info *info = a->info;
  double *x = W->x, *r = W->r, *w = W->w, *sc = W->sc;
  /* H: column j at H + j*(m+1); c, s: the rotations; g: the rotated right-hand side */
  double H[AMGD_KRYLOV_MAX_RESTART * KRY_MAXB], c[KRY_MAXB], s[KRY_MAXB], g[KRY_MAXB], y[KRY_MAXB];
  double d1[KRY_MAXB], d2[KRY_MAXB], col[KRY_MAXB + 1];

  memset(info, 0, sizeof *info);
  double beta;
  const double bnorm = sqrt(kdot(W, ordered, b, b));
  if (a->o.flags & 2) {
    amgd_d2d(x, a->dx, n * 8);
    kspmv(A, x, r, 1.0, b, -1.0);
    beta = sqrt(kdot(W, ordered, r, r));
  } else {
    amgd_vfill(x, n, 0.0);
    amgd_d2d(r, b, n * 8);
    beta = bnorm;
  }
  if (!isfinite(bnorm) || !isfinite(beta)) return -4;
  const double rt = a->o.rtol * bnorm, target = rt > a->o.atol ? rt : a->o.atol;
  info->bnorm = bnorm;
  info->r0 = info->resid = beta;
  if (beta <= target) {
    info->converged = 1;
    amgd_d2d(a->dx, x, n * 8);
    return 0;
  }
  for (;;) {
    amgd_h2d(sc + SC_ONE, &beta, 8);
    amgd_kry_scale(W->V, r, sc + SC_ONE, n);                    /* v_0 = r / beta */
    g[0] = beta;
    uint32_t k = 0;                                            /* columns of this restart */
    for (uint32_t j = 0;; j++) {
      double *vj = W->V + (uint64_t)j * ld, *zj = W->Z + (uint64_t)j * ld;
      const int nb = (int)j + 1;
      const int rc = amgd_solve_device(h, zj, vj, cyc_flags);  /* z_j = cycle(v_j) */
      if (rc != 0) return rc;
      info->cycles++;
      kspmv(A, zj, w, 0.0, NULL, 1.0);                         /* w = A z_j */
      double hn;
      if (ordered) {
        for (int i = 0; i < nb; i++) d1[i] = kdot(W, 1, W->V + (uint64_t)i * ld, w);
        amgd_h2d(sc + SC_C1, d1, (size_t)nb * 8);
        amgd_kry_axpys(w, W->V, ld, sc + SC_C1, nb, n, 0, W->part, NULL, NULL);
        for (int i = 0; i < nb; i++) d2[i] = kdot(W, 1, W->V + (uint64_t)i * ld, w);
        amgd_h2d(sc + SC_C2, d2, (size_t)nb * 8);
        amgd_kry_axpys(w, W->V, ld, sc + SC_C2, nb, n, 0, W->part, NULL, NULL);
        for (int i = 0; i < nb; i++) col[i] = d1[i] + d2[i];
        hn = sqrt(kdot(W, 1, w, NULL));
        amgd_h2d(sc + SC_HS + nb, &hn, 8);
        amgd_kry_scale(vj + ld, w, sc + SC_HS + nb, n);        /* v_{j+1} = w / h_{j+1} */
      } else {
        /* nothing here waits for the host: the update reads the dots from device memory, the
           last pass leaves d + d' with the norm behind it, and one download fetches them */
        amgd_kry_mdot(W->V, ld, w, n, nb, W->part, sc + SC_C1, NULL, NULL);
        amgd_kry_axpys(w, W->V, ld, sc + SC_C1, nb, n, 0, W->part, NULL, NULL);
        amgd_kry_mdot(W->V, ld, w, n, nb, W->part, sc + SC_C2, sc + SC_C1, sc + SC_HS);
        amgd_kry_axpys(w, W->V, ld, sc + SC_C2, nb, n, 0, W->part, sc + SC_NRM, sc + SC_HS + nb);
        amgd_kry_scale(vj + ld, w, sc + SC_HS + nb, n);
        amgd_d2h(col, sc + SC_HS, (size_t)(nb + 1) * 8);
        hn = col[nb];
      }
      col[nb] = hn;
      if (!finite_all(col, (uint32_t)nb + 1)) return -4;
      info->its++;
      amgd_route_hit(AMGD_R_KRY_IT);
      /* the earlier rotations on the new column, then the rotation that clears h_{j+1} */
      for (uint32_t i = 0; i < j; i++) {
        const double t = c[i] * col[i] + s[i] * col[i + 1];
        col[i + 1] = -s[i] * col[i] + c[i] * col[i + 1];
        col[i] = t;
      }
      const double d = sqrt(col[j] * col[j] + col[j + 1] * col[j + 1]);
      c[j] = col[j] / d;
      s[j] = col[j + 1] / d;
      col[j] = c[j] * col[j] + s[j] * col[j + 1];
      memcpy(H + (size_t)j * KRY_MAXB, col, ((size_t)j + 1) * 8);
      g[j + 1] = -s[j] * g[j];
      g[j] = c[j] * g[j];
      const double est = fabs(g[j + 1]);
      if (a->hist && info->its <= a->hist_cap) a->hist[info->its - 1] = est;
      k = j + 1;
      if (est <= target || k == m || info->its == maxit || hn == 0.) break;
    }
    /* y from the triangle, x = ((x + y_0 z_0) + y_1 z_1) + ... */
    for (uint32_t i = k; i-- > 0;) {
      double t = g[i];
      for (uint32_t l = i + 1; l < k; l++) t = t - H[(size_t)l * KRY_MAXB + i] * y[l];
      y[i] = t / H[(size_t)i * KRY_MAXB + i];
    }
    amgd_h2d(sc + SC_Y, y, (size_t)k * 8);
    amgd_kry_axpys(x, W->Z, ld, sc + SC_Y, (int)k, n, 1, W->part, NULL, NULL);
    kspmv(A, x, r, 1.0, b, -1.0);                              /* the true residual */
    beta = sqrt(kdot(W, ordered, r, r));
    if (!isfinite(beta)) return -4;
    info->resid = beta;
    if (beta <= target) { info->converged = 1; break; }
    if (info->its >= maxit) break;
    info->restarts++;
  }
  amgd_d2d(a->dx, x, n * 8);
  return info->converged ? 0 : 1;
}

API int amgd_krylov_device(amgd_hier *h, double *dx, const double *db, const amgd_krylov_opts *o,
                           amgd_krylov_info *info, double *hist, uint32_t hist_cap) {
  if (!h || !dx || !db || !o || !info || h->nlevels == 0 || h->n0 == 0) return -1;
  if (o->restart > AMGD_KRYLOV_MAX_RESTART || !(o->rtol >= 0) || !(o->atol >= 0)) return -1;
  if (h->part) return -3;
  kry_args a = {h, dx, db, *o, info, hist, hist_cap};
  if (!a.o.restart) a.o.restart = 30;
  if (!a.o.maxit) a.o.maxit = 100;
  /* the plan, then the workspace, then the iteration: each in an amgd_try of its own, so an
     unwind releases what its step allocated and nothing an earlier step keeps */
  int rc = amgd_vc_prepare(h);
  if (rc != 0) return rc;
  if (ws_ensure(h, a.o.restart) != 0) return -2;
  const int ex = amgd_get_exact();
  if (a.o.flags & 1) amgd_set_exact(1);
  amgd_kry_timer_begin();
  rc = amgd_try(kry_body, &a);
  amgd_timers_enable(1);
  amgd_kry_timer_end();
  amgd_set_exact(ex);
  g_calls++;
  g_its += info->its;
  if (g_calls % KRY_DRAIN == 0) (void)amgd_kry_timer_ms();
  if (rc < 0) amgd_sync();
  return rc;
}

API void amgd_krylov_stats(uint64_t *calls, uint64_t *its, double *ms) {
  if (calls) *calls = g_calls;
  if (its) *its = g_its;
  if (ms) *ms = amgd_kry_timer_ms();
}

/* one cycle and one level-0 product, timed like a solve (amgd_testapi.c): what an inner
   iteration costs before any orthogonalisation */
int amgd_kry_floor(amgd_hier *h, double *dx, const double *db) {
  if (!h || h->part || !h->kry || !dx || !db) return -1;
  amgd_kry_timer_begin();
  const int rc = amgd_solve_device(h, dx, db, h->nullspace ? 1 : 0);
  if (rc == 0) kspmv(h->lv[0].A.d, dx, h->kry->w, 0.0, NULL, 1.0);
  amgd_kry_timer_end();
  return rc;
}
