/*
 * amgd_testapi.c -- kernel-level test hooks of libomp_amg_amd.so.
 *
 * Exposes single device primitives on host CSR inputs so tests/test_gpu_*.py
 * can check each HIP kernel against a host restatement of the reference
 * operation it replaces (mxm, transpose, mpm, mxmpoint, apply_M, min_skel,
 * coarsen).  find_support has hooks of its own at the end of the file: amgd_test_fs_select
 * (amgd_fs_select / _amx / _ex), amgd_test_fs_expand and amgd_test_fs_claim_ext,
 * amgd_test_fs_vec (max_first, max_first2, count_gt, vdiv_guard), amgd_test_fs_mat (csc_gemv,
 * list_rowsum, bad_rows, skel_binarize, scale_diag_match) and amgd_test_find_support (the
 * whole sweep loop).  Not used by the setup path itself.
 */
#include <stdlib.h>
#include <string.h>

#include "amgd.h"

#define API __attribute__((visibility("default")))

/* The tuning switches (amgd_knob.h) by their test-side names; none of these touches the GPU.
   amgd_test_knob: set the override v, or clear it; -1: no such name */
API int amgd_test_knob(const char *name, int64_t v, int clear) {
  const int id = amgd_knob_find(name);
  if (id < 0) return -1;
  if (clear) amgd_knob_clear(id);
  else amgd_knob_set(id, v);
  return 0;
}
/* the effective value and where it comes from (0 default, 1 environment, 2 override) */
API int amgd_test_knob_get(const char *name, int64_t *value, int *source) {
  const int id = amgd_knob_find(name);
  if (id < 0) return -1;
  *value = amgd_knob(id);
  *source = amgd_knob_source(id);
  return 0;
}
/* entry `index` of the table (-1 past its end); env is NULL for a test-only switch */
API int amgd_test_knob_info(int index, const char **name, const char **env, int64_t *dflt) {
  return amgd_knob_info(index, name, env, dflt);
}
/* read the environment again, as the start of a setup does */
API void amgd_test_knobs_reread(void) { amgd_knobs_read_env(); }

typedef struct { uint32_t rn, cn; uint64_t nnz; uint64_t *ro; uint32_t *col; double *a; } hcsr;

static dcsr *up(const hcsr *H) {
  dcsr *A = dcsr_new(H->rn, H->cn, H->nnz);
  amgd_h2d(A->ro, H->ro, ((size_t)H->rn + 1) * 8);
  amgd_h2d(A->col, H->col, H->nnz * 4);
  amgd_h2d(A->a, H->a, H->nnz * 8);
  return A;
}
static void down(const dcsr *A, hcsr *H) {
  H->rn = A->rn; H->cn = A->cn; H->nnz = A->nnz;
  H->ro = (uint64_t *)malloc(((size_t)A->rn + 1) * 8);
  H->col = (uint32_t *)malloc(A->nnz * 4 + 4);
  H->a = (double *)malloc(A->nnz * 8 + 8);
  amgd_d2h(H->ro, A->ro, ((size_t)A->rn + 1) * 8);
  amgd_d2h(H->col, A->col, A->nnz * 4);
  amgd_d2h(H->a, A->a, A->nnz * 8);
}

/* op: 0 spgemm(A,B)  1 transpose(A)  2 mpm(alpha,A,beta,B)  3 mxmpoint(A,B)  4 min_skel(A)
       20 spgemm_pattern(A,B)  21 / 23 transpose by map (below) */
API int amgd_test_csr(int op, const hcsr *HA, const hcsr *HB, double alpha, double beta, hcsr *HX) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA), *B = HB ? up(HB) : NULL, *X = NULL;
  switch (op) {
    case 0: X = amgd_spgemm(A, B); break;
    case 1: X = amgd_transpose(A, NULL); break;
    case 2: X = amgd_mpm(alpha, A, beta, B); break;
    case 3: X = amgd_mxmpoint(A, B); break;
    case 4: X = amgd_min_skel(A); break;
    case 20: X = amgd_spgemm_pattern(A, B); break;
    case 5: {                     /* Q factors of the supports (rows of A) on B; X.a = packed Q */
      uint64_t tot = 0, *qoff = NULL;
      double *Q = amgd_qfactor(A, B, &qoff, &tot);
      X = (dcsr *)malloc(sizeof(dcsr));
      X->rn = A->rn; X->cn = 0; X->nnz = tot; X->ro = qoff; X->a = Q;
      X->col = (uint32_t *)amgd_alloc(tot * 4 + 4);
      amgd_memset(X->col, 0, tot * 4 + 4);
      break;
    }
    case 6: {                     /* expand_support picks on every row of A: X = pattern (ones) */
      uint8_t *all = (uint8_t *)amgd_alloc((size_t)A->rn + 1);
      amgd_memset(all, 1, (size_t)A->rn + 1);
      uint32_t *pi = NULL, *pj = NULL;
      uint64_t np = amgd_expand_pick(A, all, &pi, &pj);
      double *ones = (double *)amgd_alloc(np * 8 + 8);
      amgd_vfill(ones, np, 1.0);
      X = amgd_coo2csr(np, pi, pj, ones, A->rn, A->cn, 1);
      amgd_free(all); amgd_free(pi); amgd_free(pj); amgd_free(ones);
      break;
    }
    case 7: {                     /* Q application: Q = qfactor(A, B); X = A's pattern with
                                     values qapply(A, Q, B, u, lambda), u / lambda generated */
      uint64_t tot = 0, *qoff = NULL;
      double *Q = amgd_qfactor(A, B, &qoff, &tot);
      double *u = (double *)amgd_alloc((size_t)A->rn * 8 + 8);
      double *lam = (double *)amgd_alloc((size_t)A->cn * 8 + 8);
      double *hu = (double *)malloc((size_t)A->rn * 8 + 8), *hl = (double *)malloc((size_t)A->cn * 8 + 8);
      for (uint32_t i = 0; i < A->rn; i++) hu[i] = 0.5 + (double)(i % 3);
      for (uint32_t j = 0; j < A->cn; j++) hl[j] = 1.0 / (1.0 + (double)(j % 7));
      amgd_h2d(u, hu, (size_t)A->rn * 8);
      amgd_h2d(lam, hl, (size_t)A->cn * 8);
      free(hu); free(hl);
      X = dcsr_empty_like_pattern(A);
      amgd_qapply(A, Q, qoff, B, u, lam, X->a);
      amgd_free(Q); amgd_free(qoff); amgd_free(u); amgd_free(lam);
      break;
    }
    case 21: {                    /* T = A' with its map; A back from T as the setup driver takes
                                     it: by the map when A's rows are strictly increasing, else
                                     by the sort */
      uint64_t *perm = NULL;
      dcsr *T = amgd_transpose(A, &perm);
      X = amgd_rows_strict(A) ? amgd_untranspose_by_perm(A, perm, T->a) : amgd_transpose(T, NULL);
      amgd_free(perm);
      dcsr_free(&T);
      break;
    }
    case 23: {                    /* A' with its values gathered again through the map */
      uint64_t *perm = NULL;
      X = amgd_transpose(A, &perm);
      if (X->nnz) amgd_memset(X->a, 0xff, X->nnz * 8);
      amgd_transpose_by_perm(X, perm, A->a);
      amgd_free(perm);
      break;
    }
    default: return -2;
  }
  down(X, HX);
  dcsr_free(&A); dcsr_free(&B); dcsr_free(&X);
  return 0;
}
/* ops with a third matrix: 22 mxmpoint_sum(A, B, B2) */
API int amgd_test_csr3(int op, const hcsr *HA, const hcsr *HB, const hcsr *HB2, hcsr *HX) {
  if (amgd_rt_init(0) != 0) return -1;
  if (op != 22) return -2;
  dcsr *A = up(HA), *B = up(HB), *B2 = up(HB2);
  dcsr *X = amgd_mxmpoint_sum(A, B, B2);
  down(X, HX);
  dcsr_free(&A); dcsr_free(&B); dcsr_free(&B2); dcsr_free(&X);
  return 0;
}

/* z = alpha*y + beta*(A x) (y may be NULL) */
API int amgd_test_spmv(const hcsr *HA, const double *x, double alpha, const double *y, double beta, double *z) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  double *dx = (double *)amgd_alloc((size_t)HA->cn * 8 + 8), *dz = (double *)amgd_alloc((size_t)HA->rn * 8 + 8);
  double *dy = NULL;
  amgd_h2d(dx, x, (size_t)HA->cn * 8);
  if (y) { dy = (double *)amgd_alloc((size_t)HA->rn * 8 + 8); amgd_h2d(dy, y, (size_t)HA->rn * 8); }
  amgd_spmv(A, dx, dz, alpha, dy, beta, NULL);
  amgd_d2h(z, dz, (size_t)HA->rn * 8);
  amgd_free(dx); amgd_free(dz); if (dy) amgd_free(dy);
  dcsr_free(&A);
  return 0;
}

/* z = alpha*y + beta*(A x), f row mask, through the gather-table kernel: the matrix is
   pinned (amgd_rowmax_pin builds its tiles) for the product and unpinned after; amx != NULL:
   the fused-selection form (alpha 0, beta 1, no y / f) with each row's first largest
   product.  stats (3): table builds, tiles, direct tiles of this call. */
API int amgd_test_spmv_tab(const hcsr *HA, const double *x, double alpha, const double *y, double beta,
                           const uint8_t *f, double *z, uint64_t *amx, uint64_t *stats) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  double *dx = (double *)amgd_alloc((size_t)HA->cn * 8 + 8), *dz = (double *)amgd_alloc((size_t)HA->rn * 8 + 8);
  double *dy = NULL;
  uint8_t *df = NULL;
  uint64_t *dm = NULL;
  amgd_h2d(dx, x, (size_t)HA->cn * 8);
  if (y) { dy = (double *)amgd_alloc((size_t)HA->rn * 8 + 8); amgd_h2d(dy, y, (size_t)HA->rn * 8); }
  if (f) { df = (uint8_t *)amgd_alloc((size_t)HA->rn + 8); amgd_h2d(df, f, (size_t)HA->rn); }
  uint64_t s0[3], s1[3];
  amgd_spmv_tab_stats(s0);
  amgd_rowmax_pin(A);
  if (amx) {
    dm = (uint64_t *)amgd_alloc((size_t)HA->rn * 8 + 8);
    if (!amgd_spmv_amax(A, dx, dz, dm)) { amgd_rowmax_unpin(A); return -2; }
    amgd_d2h(amx, dm, (size_t)HA->rn * 8);
  } else {
    amgd_spmv(A, dx, dz, alpha, dy, beta, df);
  }
  amgd_spmv_tab_stats(s1);
  for (int q = 0; q < 3; q++) stats[q] = s1[q] - s0[q];
  amgd_d2h(z, dz, (size_t)HA->rn * 8);
  amgd_rowmax_unpin(A);
  amgd_free(dx); amgd_free(dz); if (dy) amgd_free(dy); if (df) amgd_free(df); if (dm) amgd_free(dm);
  dcsr_free(&A);
  return 0;
}

/* build_csr on host COO (u32 indices) */
API int amgd_test_build(uint64_t nz, const uint32_t *I, const uint32_t *J, const double *V, hcsr *HX) {
  if (amgd_rt_init(0) != 0) return -1;
  uint32_t *di = (uint32_t *)amgd_alloc(nz * 4 + 4), *dj = (uint32_t *)amgd_alloc(nz * 4 + 4);
  double *dv = (double *)amgd_alloc(nz * 8 + 8);
  amgd_h2d(di, I, nz * 4); amgd_h2d(dj, J, nz * 4); amgd_h2d(dv, V, nz * 8);
  dcsr *X = amgd_build_csr(nz, di, dj, dv);
  down(X, HX);
  dcsr_free(&X);
  amgd_free(di); amgd_free(dj); amgd_free(dv);
  return 0;
}

/* sqrt / div / 1/x on a host vector, to check IEEE rounding of the device math */
API int amgd_test_math(int op, uint64_t n, const double *a, const double *b, double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  double *da = (double *)amgd_alloc(n * 8 + 8), *db = (double *)amgd_alloc(n * 8 + 8);
  amgd_h2d(da, a, n * 8);
  amgd_h2d(db, b, n * 8);
  if (op == 0) amgd_vunary(da, n, AMGD_V_SQRT);
  else if (op == 1) amgd_vunary(da, n, AMGD_V_INV);
  else amgd_vop(da, da, db, n, AMGD_V_DIV);
  amgd_d2h(out, da, n * 8);
  amgd_free(da); amgd_free(db);
  return 0;
}

/* exact dot: mode 0 a.b, 1 a.a, 2 (a.*b).*b; plain=1 uses the one-lane loop */
extern void amgd_set_seq_plain(int on);
API double amgd_test_dot(int mode, uint64_t n, const double *a, const double *b, int plain, int exact) {
  if (amgd_rt_init(0) != 0) return 0.0 / 0.0;
  double *da = (double *)amgd_alloc(n * 8 + 8), *db = (double *)amgd_alloc(n * 8 + 8);
  amgd_h2d(da, a, n * 8);
  amgd_h2d(db, b, n * 8);
  int old = amgd_get_exact();
  amgd_set_exact(exact);
  amgd_set_seq_plain(plain);
  double r = mode == 0 ? amgd_dot(da, db, n) : mode == 1 ? amgd_dot(da, NULL, n) : amgd_dot3(da, db, n);
  amgd_set_seq_plain(0);
  amgd_set_exact(old);
  amgd_free(da); amgd_free(db);
  return r;
}

API void amgd_test_free(hcsr *H) {
  free(H->ro); free(H->col); free(H->a);
  H->ro = NULL; H->col = NULL; H->a = NULL;
}

/* interp_lmop counters: [fast, general, dirty-prefix, misses, pruned] */
API void amgd_test_lmop_stats(uint64_t *out, int reset) {
  amgd_lmop_stats(out);
  if (reset) amgd_lmop_stats_reset();
}

/* huge-support Q factor: [sparse, fallback, split] counters */
API void amgd_test_qf_stats(uint64_t *out) {
  unsigned long st[3];
  amgd_qfactor_stats(st);
  out[0] = st[0];
  out[1] = st[1];
  out[2] = st[2];
}

/* whole-matrix SpMVs that ran row-sharded (multi-GPU) since the library loaded */
extern uint64_t amgd_spmv_shard_calls(void);
/* cols_masked(A, mask) and transpose(rows_masked(B, mask)) for the same mask: equal */
API int amgd_test_cols_masked(const hcsr *HA, const uint8_t *hmask, hcsr *HX) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  uint8_t *m = (uint8_t *)amgd_alloc((size_t)A->cn + 1);
  amgd_h2d(m, hmask, A->cn);
  dcsr *X = amgd_cols_masked(A, m);
  down(X, HX);
  dcsr_free(&X); dcsr_free(&A);
  amgd_free(m);
  return 0;
}
/* Q factors taken by copy from the previous iteration / factored, since the last call */
API void amgd_test_qf_reuse_stats(uint64_t *out) {
  static uint64_t r0 = 0, f0 = 0;
  uint64_t r, f;
  amgd_qfactor_reuse_stats(&r, &f);
  out[0] = r - r0; out[1] = f - f0;
  r0 = r; f0 = f;
}
/* cap on live device bytes (0: none): the out-of-HBM path without filling 288 GB */
API void amgd_test_hbm_cap(uint64_t bytes) { amgd_knob_set(AMGD_K_HBM_CAP, (int64_t)bytes); }
API uint64_t amgd_test_pool_inuse(void) { return amgd_pool_bytes_in_use(); }

/* one bare partitioned-mode collective (the collective guard's tests): kind 0 an allgatherv
   of `bytes` per rank, 1 an alltoallv of `bytes` to every peer (expecting `expect` bytes
   from each); returns 0 */
API int amgd_test_comm(int kind, uint64_t bytes, uint64_t expect) {
  const int N = amgd_pcomm_size(), me = amgd_pcomm_rank();
  uint64_t *so = (uint64_t *)malloc(8 * ((size_t)N + 1)), *ro = (uint64_t *)malloc(8 * ((size_t)N + 1));
  for (int p = 0; p <= N; p++) { so[p] = bytes * p; ro[p] = (kind ? expect : bytes) * p; }
  char *sb = (char *)amgd_alloc(bytes * N + 16), *rb = (char *)amgd_alloc(ro[N] + 16);
  amgd_memset(sb, me + 1, bytes * N);
  if (kind == 0) {
    void *b = sb;
    amgd_allgatherv(1, &b, so);
  } else {
    amgd_pcomm_alltoallv(sb, so, rb, ro);
  }
  amgd_sync();
  amgd_free(sb); amgd_free(rb);
  free(so); free(ro);
  return 0;
}
/* kernel-route counters since the last reset (out: AMGD_R_N entries) */
API void amgd_test_route_stats(uint64_t *out, int reset) {
  for (int r = 0; r < AMGD_R_N; r++) out[r] = amgd_route_ctr[r];
  if (reset) memset(amgd_route_ctr, 0, sizeof amgd_route_ctr);
}
API uint64_t amgd_test_spmv_shard_calls(void) { return amgd_spmv_shard_calls(); }

/* partitioned setup: [interp_lmop calls on gathered data, calls with a dirty prefix,
   eager exchanges, eager exchanges that took the exact second round] of the last setup(s) */
API void amgd_test_part_stats(uint64_t *out) {
  amgd_part_stats(out);
  pm_eager_stats(out + 2, out + 3);
}
/* forced rare paths: every interp_lmop on gathered data; a fixed eager slot (bytes, 0: adaptive) */
API void amgd_test_part_force(int lmop_gather, int64_t eager_slot) {
  if (lmop_gather < 0) amgd_knob_clear(AMGD_K_PART_LMOP_GATHER);
  else amgd_knob_set(AMGD_K_PART_LMOP_GATHER, lmop_gather);
  if (eager_slot < 0) amgd_knob_clear(AMGD_K_EAGER_SLOT);
  else amgd_knob_set(AMGD_K_EAGER_SLOT, eager_slot);
}
API void amgd_test_spat_stats(uint64_t *out3) { amgd_spat_stats(out3); }
API void amgd_test_spgemm_sym(int mode) { if (mode < 0) amgd_spgemm_sym_drop(); else amgd_spgemm_sym_next(mode); }
API void amgd_test_spgemm_sym_stats(uint64_t *kept, uint64_t *reused) { amgd_spgemm_sym_stats(kept, reused); }
/* amgd_spmv with every option: x NULL = ordered row sums, y / f optional (f: u8 row mask) */
API int amgd_test_spmv_f(const hcsr *HA, const double *x, double alpha, const double *y, double beta,
                         const uint8_t *f, double *z) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  double *dx = NULL, *dy = NULL, *dz = (double *)amgd_alloc((size_t)HA->rn * 8 + 8);
  uint8_t *df = NULL;
  if (x) { dx = (double *)amgd_alloc((size_t)HA->cn * 8 + 8); amgd_h2d(dx, x, (size_t)HA->cn * 8); }
  if (y) { dy = (double *)amgd_alloc((size_t)HA->rn * 8 + 8); amgd_h2d(dy, y, (size_t)HA->rn * 8); }
  if (f) { df = (uint8_t *)amgd_alloc((size_t)HA->rn + 8); amgd_h2d(df, f, HA->rn); }
  amgd_spmv(A, dx, dz, alpha, dy, beta, df);
  amgd_d2h(z, dz, (size_t)HA->rn * 8);
  if (dx) amgd_free(dx);
  if (dy) amgd_free(dy);
  if (df) amgd_free(df);
  amgd_free(dz);
  dcsr_free(&A);
  return 0;
}

/* amgd_spmv_rows: z[list[r]] = (A x)[list[r]] (x NULL: row sums); other rows of z keep
   their input values */
API int amgd_test_spmv_rows(const hcsr *HA, const uint32_t *list, uint32_t n, const double *x, double *z) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  double *dx = NULL, *dz = (double *)amgd_alloc((size_t)HA->rn * 8 + 8);
  uint32_t *dl = (uint32_t *)amgd_alloc((size_t)n * 4 + 8);
  if (x) { dx = (double *)amgd_alloc((size_t)HA->cn * 8 + 8); amgd_h2d(dx, x, (size_t)HA->cn * 8); }
  amgd_h2d(dz, z, (size_t)HA->rn * 8);
  amgd_h2d(dl, list, (size_t)n * 4);
  amgd_spmv_rows(A, dl, n, dx, dz);
  amgd_d2h(z, dz, (size_t)HA->rn * 8);
  if (dx) amgd_free(dx);
  amgd_free(dz); amgd_free(dl);
  dcsr_free(&A);
  return 0;
}

/* SpMV micro-benchmark: a generated matrix (amgd_bench_matrix), reps products timed
   with HIP events on the library stream; with_x = 0: ordered row sums (no gather).
   Returns ms per product and the matrix's nnz. */
extern dcsr *amgd_bench_matrix(uint32_t rn, uint32_t cn, uint32_t len0, uint32_t len1, uint32_t gap);
API double amgd_test_spmv_bench(uint32_t rn, uint32_t cn, uint32_t len0, uint32_t len1, uint32_t gap,
                                int with_x, int reps, uint64_t *nnz) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = amgd_bench_matrix(rn, cn, len0, len1, gap);
  double *x = (double *)amgd_alloc((size_t)cn * 8 + 8), *z = (double *)amgd_alloc((size_t)rn * 8 + 8);
  amgd_vfill(x, cn, 0.5);
  amgd_spmv(A, with_x ? x : NULL, z, 0.0, NULL, 1.0, NULL);   /* warm */
  amgd_timer_reset();
  for (int r = 0; r < reps; r++) {
    amgd_timer_start(7);
    amgd_spmv(A, with_x ? x : NULL, z, 0.0, NULL, 1.0, NULL);
    amgd_timer_stop(7);
  }
  double ms = amgd_timer_ms(7) / reps;
  *nnz = A->nnz;
  amgd_free(x); amgd_free(z);
  dcsr_free(&A);
  return ms;
}

/* ---------------------------------------------------------------------------
 * Row-partitioned primitives (amgd_part.h), one pm_* call per hook call
 * (tests/test_gpu_part_prims.py).  Every rank passes the WHOLE host operands and the host
 * split arrays (N + 1 entries) of their row and column spaces; the hook fills its own
 * `apart`s from the splits (any contiguous split, not only apart_even's), uploads rows
 * [split[me], split[me + 1]) as the local dcsr with global columns, runs the call and
 * hands back the rank's local block (X) or the whole vector (z).  a_nocol / b_nocol:
 * the operand is uploaded with col == NULL (the values-only pseudo-matrix of the Q factors).
 * Every rank must make the same sequence of calls.  Not used by the setup path.
 * --------------------------------------------------------------------------- */
#include "amgd_part.h"

typedef struct {
  const hcsr *A, *B;
  const uint32_t *ars, *acs, *brs, *bcs;     /* row / column splits of A and B */
  int32_t a_nocol, b_nocol, iarg, pad_;
  double alpha, beta;
  const double *x, *y;                       /* whole host vectors (op-specific) */
  const uint8_t *f, *vr, *vc;                /* whole host masks */
  const uint32_t *li, *lj;                   /* lists / COO indices */
  uint64_t nl, nl2;
  hcsr X;                                    /* out: local block (amgd_test_free it) */
  double *z, *z2;                            /* in/out: whole vectors (caller's) */
  uint32_t *so_r, *so_c;                     /* out: induced splits (N + 1, caller's) */
  double scalar;                             /* out */
} pm_targs;

static void fill_part(apart *P, const uint32_t *split) {
  P->N = amgd_pcomm_size();
  P->split = (uint32_t *)split;
  P->n = split[P->N];
}
static dcsr *up_rows(const hcsr *H, const apart *P, int nocol) {
  const int me = amgd_pcomm_rank();
  const uint32_t lo = P->split[me], hi = P->split[me + 1], rn = hi - lo;
  const uint64_t k0 = H->ro[lo], nz = H->ro[hi] - k0;
  dcsr *A = dcsr_new(rn, H->cn, nz);
  uint64_t *ro = (uint64_t *)malloc(((size_t)rn + 1) * 8);
  for (uint32_t i = 0; i <= rn; i++) ro[i] = H->ro[lo + i] - k0;
  amgd_h2d(A->ro, ro, ((size_t)rn + 1) * 8);
  free(ro);
  if (nocol) { amgd_free(A->col); A->col = NULL; }
  else amgd_h2d(A->col, H->col + k0, nz * 4);
  amgd_h2d(A->a, H->a + k0, nz * 8);
  return A;
}
/* like down(); a missing col / a array comes back as NULL */
static void down_opt(const dcsr *A, hcsr *H) {
  H->rn = A->rn; H->cn = A->cn; H->nnz = A->nnz;
  H->ro = (uint64_t *)malloc(((size_t)A->rn + 1) * 8);
  amgd_d2h(H->ro, A->ro, ((size_t)A->rn + 1) * 8);
  H->col = NULL; H->a = NULL;
  if (A->col) { H->col = (uint32_t *)malloc(A->nnz * 4 + 4); amgd_d2h(H->col, A->col, A->nnz * 4); }
  if (A->a) { H->a = (double *)malloc(A->nnz * 8 + 8); amgd_d2h(H->a, A->a, A->nnz * 8); }
}
static void *up_buf(const void *h, size_t bytes) {
  if (!h) return NULL;
  void *d = amgd_alloc(bytes + 8);
  amgd_h2d(d, h, bytes);
  return d;
}

enum { PT_TRANSPOSE = 0, PT_SPGEMM, PT_HALO, PT_SUB_MAT, PT_MPM, PT_MXMPOINT, PT_DROP_ZEROS, PT_ROWS_MASKED,
       PT_DIAG_OP, PT_DIAG_OP2, PT_GATHER_FULL, PT_GATHER_PATTERN, PT_ZERO_ENTRIES, PT_COO_ONES, PT_KPOS,
       PT_SPMV = 20, PT_SPMVT, PT_COLSUM, PT_DIAG, PT_ROWSUM_SQ_INV, PT_FRO,
       PT_LIST_SYNC = 30, PT_LIST_SYNC2, PT_LIST_ROWSUM, PT_LIST_ROWSUM2,
       PT_INDUCED = 40, PT_ROUTE_COO };

API int amgd_test_pm(int op, pm_targs *t) {
  if (amgd_rt_init(0) != 0) return -1;
  const int N = amgd_pcomm_size();
  apart ar, ac, br, bc;
  memset(&t->X, 0, sizeof t->X);
  if (t->ars) fill_part(&ar, t->ars);
  if (t->acs) fill_part(&ac, t->acs);
  if (t->brs) fill_part(&br, t->brs);
  if (t->bcs) fill_part(&bc, t->bcs);
  pmat *A = t->A ? pm_new(up_rows(t->A, &ar, t->a_nocol), &ar, &ac) : NULL;
  pmat *B = t->B ? pm_new(up_rows(t->B, &br, t->b_nocol), &br, &bc) : NULL;
  const uint32_t rn = t->ars ? ar.n : 0, cn = t->acs ? ac.n : 0;
  pmat *X = NULL;
  int rc = 0;
  switch (op) {
    case PT_TRANSPOSE: X = pm_transpose(A); break;
    case PT_SPGEMM: X = pm_spgemm(A, B, t->iarg); break;
    case PT_HALO: {                /* X = the global-row view of B beside the rows A references */
      dcsr *E = pm_halo_rows(B, A->m);
      down_opt(E, &t->X);
      pm_ext_free(&E);
      break;
    }
    case PT_SUB_MAT: {
      uint8_t *vr = (uint8_t *)up_buf(t->vr, rn), *vc = (uint8_t *)up_buf(t->vc, cn);
      apart *ro = apart_induced(&ar, vr), *co = apart_induced(&ac, vc);
      X = pm_sub_mat(A, vr, vc, ro, co);
      memcpy(t->so_r, ro->split, 4 * ((size_t)N + 1));
      memcpy(t->so_c, co->split, 4 * ((size_t)N + 1));
      down_opt(X->m, &t->X);
      pm_free(&X);
      apart_free(&ro); apart_free(&co);
      amgd_free(vr); amgd_free(vc);
      break;
    }
    case PT_MPM: X = pm_mpm(t->alpha, A, t->beta, B); break;
    case PT_MXMPOINT: X = pm_mxmpoint(A, B); break;
    case PT_DROP_ZEROS: X = pm_drop_zeros(A); break;
    case PT_ROWS_MASKED: {
      uint8_t *f = (uint8_t *)up_buf(t->f, rn);
      X = pm_rows_masked(A, f);
      amgd_free(f);
      break;
    }
    case PT_DIAG_OP: case PT_DIAG_OP2: {   /* x: the row-space vector, y: the column-space one */
      double *dl = (double *)up_buf(t->x, 8 * (size_t)rn), *dr = (double *)up_buf(t->y, 8 * (size_t)cn);
      if (op == PT_DIAG_OP) pm_diag_op(A, dl, t->iarg);
      else pm_diag_op2(A, dl, dr, t->iarg);
      down_opt(A->m, &t->X);
      amgd_free(dl); amgd_free(dr);
      break;
    }
    case PT_GATHER_FULL: case PT_GATHER_PATTERN: {
      dcsr *F = op == PT_GATHER_FULL ? pm_gather_full(A) : pm_gather_pattern(A);
      down_opt(F, &t->X);
      dcsr_free(&F);
      break;
    }
    case PT_ZERO_ENTRIES: {
      uint32_t *ri = (uint32_t *)up_buf(t->li, 4 * t->nl), *cj = (uint32_t *)up_buf(t->lj, 4 * t->nl);
      pm_zero_entries(A, ri, cj, t->nl);
      down_opt(A->m, &t->X);
      amgd_free(ri); amgd_free(cj);
      break;
    }
    case PT_COO_ONES: {
      uint32_t *ri = (uint32_t *)up_buf(t->li, 4 * t->nl), *cj = (uint32_t *)up_buf(t->lj, 4 * t->nl);
      X = pm_coo_ones(ri, cj, t->nl, &ar, &ac);
      amgd_free(ri); amgd_free(cj);
      break;
    }
    case PT_KPOS: {                /* X = A's local block with a[e] = kpos[e] */
      pmat *T = pm_transpose(A);
      dcsr *E = pm_halo_rows(T, A->m);
      uint32_t *kp = pm_kpos(A, E);
      uint32_t *h = (uint32_t *)malloc(4 * A->m->nnz + 4);
      amgd_d2h(h, kp, 4 * A->m->nnz);
      down_opt(A->m, &t->X);
      for (uint64_t e = 0; e < A->m->nnz; e++) t->X.a[e] = (double)h[e];
      free(h);
      amgd_free(kp);
      pm_ext_free(&E);
      pm_free(&T);
      break;
    }
    case PT_SPMV: case PT_SPMVT: case PT_COLSUM: case PT_DIAG: case PT_ROWSUM_SQ_INV: {
      /* z comes in pre-filled: the segments of the other ranks must be overwritten */
      double *x = (double *)up_buf(t->x, 8 * (size_t)cn), *y = (double *)up_buf(t->y, 8 * (size_t)rn);
      uint8_t *f = (uint8_t *)up_buf(t->f, rn);
      double *z = (double *)up_buf(t->z, 8 * (size_t)rn);
      if (op == PT_SPMV) pm_spmv(A, x, z, t->alpha, y, t->beta, f);
      else if (op == PT_SPMVT) pm_spmvt(A, x, z);
      else if (op == PT_COLSUM) pm_colsum(A, z);
      else if (op == PT_DIAG) pm_diag(A, z);
      else pm_rowsum_sq_inv(A, z);
      amgd_d2h(t->z, z, 8 * (size_t)rn);
      amgd_free(x); amgd_free(y); amgd_free(f); amgd_free(z);
      break;
    }
    case PT_FRO: t->scalar = pm_fro_minus_eye(A); break;
    case PT_LIST_SYNC: case PT_LIST_SYNC2: {   /* (z, li, nl, ars) and (z2, lj, nl2, brs) */
      double *z[2] = {(double *)up_buf(t->z, 8 * (size_t)ar.n), NULL};
      uint32_t *l[2] = {(uint32_t *)up_buf(t->li, 4 * t->nl), NULL};
      if (op == PT_LIST_SYNC) {
        pm_list_sync(z[0], l[0], (uint32_t)t->nl, &ar);
      } else {
        z[1] = (double *)up_buf(t->z2, 8 * (size_t)br.n);
        l[1] = (uint32_t *)up_buf(t->lj, 4 * t->nl2);
        const uint32_t n[2] = {(uint32_t)t->nl, (uint32_t)t->nl2};
        const apart *P[2] = {&ar, &br};
        pm_list_sync_n(2, z, (const uint32_t *const *)l, n, P);
        amgd_d2h(t->z2, z[1], 8 * (size_t)br.n);
      }
      amgd_d2h(t->z, z[0], 8 * (size_t)ar.n);
      amgd_free(z[0]); amgd_free(z[1]); amgd_free(l[0]); amgd_free(l[1]);
      break;
    }
    case PT_LIST_ROWSUM: case PT_LIST_ROWSUM2: {
      double *z = (double *)up_buf(t->z, 8 * (size_t)ar.n), *z2 = NULL;
      uint32_t *la = (uint32_t *)up_buf(t->li, 4 * t->nl), *lb = NULL;
      if (op == PT_LIST_ROWSUM) {
        pm_list_rowsum(A, la, (uint32_t)t->nl, z);
      } else {
        z2 = (double *)up_buf(t->z2, 8 * (size_t)br.n);
        lb = (uint32_t *)up_buf(t->lj, 4 * t->nl);
        pm_list_rowsum2(A, la, z, B, lb, z2, (uint32_t)t->nl);
        amgd_d2h(t->z2, z2, 8 * (size_t)br.n);
      }
      amgd_d2h(t->z, z, 8 * (size_t)ar.n);
      amgd_free(z); amgd_free(z2); amgd_free(la); amgd_free(lb);
      break;
    }
    case PT_INDUCED: {
      uint8_t *f = (uint8_t *)up_buf(t->f, rn);
      apart *Q = apart_induced(&ar, f);
      memcpy(t->so_r, Q->split, 4 * ((size_t)N + 1));
      apart_free(&Q);
      amgd_free(f);
      break;
    }
    case PT_ROUTE_COO: {           /* this rank's nl entries (li, lj, x); out: X.nnz entries with
                                      the rows in X.ro (widened to u64), columns X.col, values X.a */
      uint32_t *I = (uint32_t *)amgd_alloc(4 * t->nl + 8), *J = (uint32_t *)amgd_alloc(4 * t->nl + 8);
      double *V = (double *)amgd_alloc(8 * t->nl + 8);
      amgd_h2d(I, t->li, 4 * t->nl); amgd_h2d(J, t->lj, 4 * t->nl); amgd_h2d(V, t->x, 8 * t->nl);
      uint32_t *Io = NULL, *Jo = NULL;
      double *Vo = NULL;
      const uint64_t m = pm_route_coo(t->nl, I, J, V, &ar, &Io, &Jo, &Vo);
      uint32_t *hi = (uint32_t *)malloc(4 * m + 4);
      t->X.rn = 0; t->X.cn = 0; t->X.nnz = m;
      t->X.ro = (uint64_t *)malloc(8 * m + 8);
      t->X.col = (uint32_t *)malloc(4 * m + 4);
      t->X.a = (double *)malloc(8 * m + 8);
      amgd_d2h(hi, Io, 4 * m); amgd_d2h(t->X.col, Jo, 4 * m); amgd_d2h(t->X.a, Vo, 8 * m);
      for (uint64_t k = 0; k < m; k++) t->X.ro[k] = hi[k];
      free(hi);
      amgd_free(I); amgd_free(J); amgd_free(V); amgd_free(Io); amgd_free(Jo); amgd_free(Vo);
      break;
    }
    default: rc = -2;
  }
  if (X) { down_opt(X->m, &t->X); pm_free(&X); }
  pm_free(&A);
  pm_free(&B);
  amgd_sync();
  return rc;
}

/* pm_allgather_dyn with one of four persistent call-site states (state < 0: a fresh one):
   mine = this rank's `bytes` (host); out (host, cap bytes) gets the concatenation; slot_after:
   the state's slot after the call */
API int amgd_test_pm_eager(int state, const void *mine, uint64_t bytes, uint64_t user, uint64_t *len,
                           uint64_t *users, uint64_t *total, void *out, uint64_t cap, uint64_t *slot_after) {
  static pm_eager st[4];
  if (amgd_rt_init(0) != 0) return -1;
  pm_eager fresh = {0, 0}, *e = state < 0 ? &fresh : &st[state & 3];
  char *d = (char *)amgd_alloc(bytes + 8);
  amgd_h2d(d, mine, bytes);
  char *o = pm_allgather_dyn(e, d, bytes, user, len, users, total);
  const int ok = *total <= cap;
  if (ok) amgd_d2h(out, o, *total);
  *slot_after = e->slot;
  amgd_free(o); amgd_free(d);
  amgd_sync();
  return ok ? 0 : -3;
}
API void amgd_test_pm_eager_new_setup(void) { pm_eager_new_setup(); }

/* ---------------------------------------------------------------------------
 * find_support (amgd_setup.c:407) piece by piece (tests/test_gpu_fs.py): the selection in
 * its three forms, the incremental sweeps' expansion, the reductions and small kernels that
 * feed the loop's host decisions, and the loop itself.  Whole host CSR / vectors in, host
 * arrays out.
 * --------------------------------------------------------------------------- */
static uint32_t *up_u32(const uint32_t *h, size_t n) {
  uint32_t *d = (uint32_t *)amgd_alloc(n * 4 + 8);
  if (n) amgd_h2d(d, h, n * 4);
  return d;
}
static double *up_f64(const double *h, size_t n) {
  double *d = (double *)amgd_alloc(n * 8 + 8);
  if (n) amgd_h2d(d, h, n * 8);
  return d;
}

/* One selection sweep on R (nf x nc).  variant 0: amgd_fs_select; 1: amgd_spmv_amax(R', rs)
   then amgd_fs_select_amx (out3[2] = what amgd_spmv_amax returned; 0: no selection is made);
   2: amgd_fs_select_ex on a copy of rows [c0, c1) of R' with perm NULL, w + c0, sumR + c0 and
   resum 0, as the partitioned driver calls it.  pin: R and R' (the window) pinned as
   find_support pins them.  rs (nf), sumR (nc) in / out; w (nc) in; sel_i / sel_j: nc entries;
   out3 = {selections, nremoved, amax delivered}; Ra / Rta: R's values and the whole R''s
   values (CSC order) after the call. */
API int amgd_test_fs_select(int variant, const hcsr *HR, double *rs, const double *w, double *sumR,
                            double thr, int pin, uint32_t c0, uint32_t c1, uint32_t *sel_i,
                            uint32_t *sel_j, uint32_t *out3, double *Ra, double *Rta) {
  if (amgd_rt_init(0) != 0) return -1;
  const uint32_t nf = HR->rn, nc = HR->cn;
  if (variant < 0 || variant > 2 || (variant == 2 && (c0 > c1 || c1 > nc))) return -2;
  dcsr *R = up(HR);
  uint64_t *perm = NULL;
  dcsr *Rt = amgd_transpose(R, &perm), *Win = NULL;
  double *drs = up_f64(rs, nf), *dw = up_f64(w, nc), *dsum = up_f64(sumR, nc);
  uint32_t *si = (uint32_t *)amgd_alloc((size_t)nc * 4 + 8), *sj = (uint32_t *)amgd_alloc((size_t)nc * 4 + 8);
  uint32_t nsel = 0, nrem = 0;
  uint64_t k0 = 0;
  out3[2] = 0;
  if (variant == 2) {                       /* rows [c0, c1) of R' as a matrix of its own */
    hcsr HT;
    down(Rt, &HT);
    k0 = HT.ro[c0];
    const uint32_t wn = c1 - c0;
    Win = dcsr_new(wn, nf, HT.ro[c1] - k0);
    uint64_t *ro = (uint64_t *)malloc(((size_t)wn + 1) * 8);
    for (uint32_t i = 0; i <= wn; i++) ro[i] = HT.ro[c0 + i] - k0;
    amgd_h2d(Win->ro, ro, ((size_t)wn + 1) * 8);
    if (Win->nnz) {
      amgd_h2d(Win->col, HT.col + k0, Win->nnz * 4);
      amgd_h2d(Win->a, HT.a + k0, Win->nnz * 8);
    }
    free(ro);
    amgd_test_free(&HT);
  }
  if (pin) { amgd_rowmax_pin(R); amgd_rowmax_pin(Win ? Win : Rt); }
  if (variant == 0) {
    nsel = amgd_fs_select(R, Rt, perm, drs, dw, dsum, thr, si, sj, &nrem);
  } else if (variant == 1) {
    uint64_t *amx = (uint64_t *)amgd_alloc((size_t)nc * 8 + 8);
    double *wp = (double *)amgd_alloc((size_t)nc * 8 + 8);
    out3[2] = (uint32_t)amgd_spmv_amax(Rt, drs, wp, amx);
    if (out3[2]) nsel = amgd_fs_select_amx(R, Rt, perm, drs, dw, dsum, thr, amx, si, sj, &nrem);
    amgd_free(amx); amgd_free(wp);
  } else {
    nsel = amgd_fs_select_ex(R, Win, NULL, drs, dw + c0, dsum + c0, thr, si, sj, &nrem, c0, 0);
  }
  amgd_sync();
  if (pin) { amgd_rowmax_unpin(R); amgd_rowmax_unpin(Win ? Win : Rt); }
  out3[0] = nsel; out3[1] = nrem;
  if (nsel > nc) nsel = nc;
  if (nsel) { amgd_d2h(sel_i, si, (size_t)nsel * 4); amgd_d2h(sel_j, sj, (size_t)nsel * 4); }
  if (nf) amgd_d2h(rs, drs, (size_t)nf * 8);
  if (nc) amgd_d2h(sumR, dsum, (size_t)nc * 8);
  if (R->nnz) { amgd_d2h(Ra, R->a, R->nnz * 8); amgd_d2h(Rta, Rt->a, Rt->nnz * 8); }
  if (Win && Win->nnz) amgd_d2h(Rta + k0, Win->a, Win->nnz * 8);
  amgd_free(drs); amgd_free(dw); amgd_free(dsum); amgd_free(si); amgd_free(sj); amgd_free(perm);
  dcsr_free(&R); dcsr_free(&Rt);
  if (Win) dcsr_free(&Win);
  return 0;
}

/* amgd_fs_expand on the listed rows of M: stamp (M's columns) in / out, out: cap entries;
   res = {count, the word behind out[cap - 1] (stays 0xffffffff)} */
API int amgd_test_fs_expand(const hcsr *HM, const uint32_t *list, uint32_t n, uint32_t *stamp, uint32_t tag,
                            uint32_t cap, int pin, uint32_t *out, uint32_t *res) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *M = up(HM);
  uint32_t *dl = up_u32(list, n), *ds = up_u32(stamp, HM->cn);
  uint32_t *dout = (uint32_t *)amgd_alloc((size_t)cap * 4 + 8);
  amgd_memset(dout, 0xff, (size_t)cap * 4 + 8);
  if (pin) amgd_rowmax_pin(M);
  res[0] = amgd_fs_expand(M, dl, n, ds, tag, dout, cap);
  amgd_sync();
  if (pin) amgd_rowmax_unpin(M);
  if (cap) amgd_d2h(out, dout, (size_t)cap * 4);
  amgd_d2h(res + 1, dout + cap, 4);
  if (HM->cn) amgd_d2h(stamp, ds, (size_t)HM->cn * 4);
  amgd_free(dl); amgd_free(ds); amgd_free(dout);
  dcsr_free(&M);
  return 0;
}
/* amgd_fs_claim_ext: ids (n) claimed into out behind its first `have` entries; stamp: ns words */
API int amgd_test_fs_claim_ext(const uint32_t *ids, uint64_t n, uint32_t *stamp, uint32_t ns, uint32_t tag,
                               uint32_t have, uint32_t cap, uint32_t *out, uint32_t *res) {
  if (amgd_rt_init(0) != 0) return -1;
  uint32_t *di = up_u32(ids, n), *ds = up_u32(stamp, ns);
  uint32_t *dout = (uint32_t *)amgd_alloc((size_t)cap * 4 + 8);
  amgd_memset(dout, 0xff, (size_t)cap * 4 + 8);
  if (cap) amgd_h2d(dout, out, (size_t)cap * 4);
  res[0] = amgd_fs_claim_ext(di, n, ds, tag, dout, have, cap);
  amgd_sync();
  if (cap) amgd_d2h(out, dout, (size_t)cap * 4);
  amgd_d2h(res + 1, dout + cap, 4);
  if (ns) amgd_d2h(stamp, ds, (size_t)ns * 4);
  amgd_free(di); amgd_free(ds); amgd_free(dout);
  return 0;
}

/* vectors: op 0 max_first(a) -> outd[0], outu[0]; 1 max_first2(a, b) -> outd[0], outu[0],
   outd[1] = max(b); 2 count_gt(a, thr) -> outu[0], outd[0] = max; 3 outd[0..n) = vdiv_guard(a, b) */
API int amgd_test_fs_vec(int op, uint64_t n, const double *a, const double *b, double thr, double *outd,
                         uint64_t *outu) {
  if (amgd_rt_init(0) != 0) return -1;
  double *da = up_f64(a, n), *db = b ? up_f64(b, n) : NULL;
  int rc = 0;
  switch (op) {
    case 0: outd[0] = amgd_max_first(da, n, outu); break;
    case 1: outd[0] = amgd_max_first2(da, db, n, outu, outd + 1); break;
    case 2: outu[0] = amgd_count_gt(da, n, thr, outd); break;
    case 3: {
      double *r = (double *)amgd_alloc(n * 8 + 8);
      amgd_vdiv_guard(r, da, db, n);
      if (n) amgd_d2h(outd, r, n * 8);
      amgd_free(r);
      break;
    }
    default: rc = -2;
  }
  amgd_sync();
  amgd_free(da);
  if (db) amgd_free(db);
  return rc;
}
/* matrices: op 0 z (cn) = csc_gemv(A', map, A's values, x or NULL); 1 list_rowsum(A, list, nl,
   z, iarg) with z (rn) in / out; 2 bad_rows(A) -> mask (rn), cnt[0]; 3 skel_binarize(A, iarg)
   -> avals; 4 scale_diag_match(A, x, y) -> avals */
API int amgd_test_fs_mat(int op, const hcsr *HA, const double *x, const double *y, const uint32_t *list,
                         uint32_t nl, int iarg, double *z, uint8_t *mask, uint32_t *cnt, double *avals) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *A = up(HA);
  int rc = 0;
  switch (op) {
    case 0: {
      uint64_t *perm = NULL;
      dcsr *T = amgd_transpose(A, &perm);
      double *dx = x ? up_f64(x, A->rn) : NULL, *dz = (double *)amgd_alloc((size_t)A->cn * 8 + 8);
      amgd_csc_gemv(T, perm, A->a, dx, dz);
      if (A->cn) amgd_d2h(z, dz, (size_t)A->cn * 8);
      if (dx) amgd_free(dx);
      amgd_free(dz); amgd_free(perm);
      dcsr_free(&T);
      break;
    }
    case 1: {
      double *dz = up_f64(z, A->rn);
      uint32_t *dl = up_u32(list, nl);
      amgd_list_rowsum(A, dl, nl, dz, iarg);
      if (A->rn) amgd_d2h(z, dz, (size_t)A->rn * 8);
      amgd_free(dz); amgd_free(dl);
      break;
    }
    case 2: {
      uint8_t *bad = amgd_bad_rows(A, cnt);
      if (A->rn) amgd_d2h(mask, bad, A->rn);
      amgd_free(bad);
      break;
    }
    case 3: case 4: {
      if (op == 3) {
        amgd_skel_binarize(A, iarg);
      } else {
        double *dv = up_f64(x, A->rn), *dw = up_f64(y, A->rn);
        amgd_scale_diag_match(A, dv, dw);
        amgd_free(dv); amgd_free(dw);
      }
      if (A->nnz) amgd_d2h(avals, A->a, A->nnz * 8);
      break;
    }
    default: rc = -2;
  }
  amgd_sync();
  dcsr_free(&A);
  return rc;
}

/* the whole loop: Sk = find_support(R, goal); first: {rs, w, tmp, w2} (host) handed in as the
   caller's first-sweep products, or NULL; res = {sweeps, first UB() site or 0} */
extern dcsr *amgd_test_hook_find_support(dcsr *R, double goal, const double *const *first, uint32_t *ub);
API int amgd_test_find_support(const hcsr *HR, double goal, const double *const *first, hcsr *HX,
                               uint32_t *res) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *R = up(HR);
  const double *df[4] = {NULL, NULL, NULL, NULL};
  if (first) {
    df[0] = up_f64(first[0], HR->rn); df[1] = up_f64(first[1], HR->cn);
    df[2] = up_f64(first[2], HR->rn); df[3] = up_f64(first[3], HR->cn);
  }
  const uint64_t s0 = amgd_route_ctr[AMGD_R_FS_SWEEP];
  dcsr *Sk = amgd_test_hook_find_support(R, goal, first ? df : NULL, res + 1);
  res[0] = (uint32_t)(amgd_route_ctr[AMGD_R_FS_SWEEP] - s0);
  down(Sk, HX);
  dcsr_free(&Sk);
  for (int q = 0; q < 4; q++) if (df[q]) amgd_free((void *)df[q]);
  return 0;
}

/* ---------------------------------------------------------------------------
 * The two consumers of the Q factors (tests/test_gpu_weights.py) on the caller's operands.
 * --------------------------------------------------------------------------- */
/* out (nnz(Wt) doubles) = amgd_qapply(Wt, amgd_qfactor(Wt, A), Bt, u, lambda); Bt has one row
   per support (row of Wt), u one entry per support, lambda one per column of Wt.  out starts
   as a NaN pattern on the device: an entry no kernel wrote comes back as one. */
API int amgd_test_qapply(const hcsr *HWt, const hcsr *HA, const hcsr *HBt, const double *u,
                         const double *lambda, double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (HBt->rn != HWt->rn || HA->rn != HWt->cn) return -2;
  dcsr *Wt = up(HWt), *A = up(HA), *Bt = up(HBt);
  uint64_t tot = 0, *qoff = NULL;
  double *Q = amgd_qfactor(Wt, A, &qoff, &tot);
  double *du = up_f64(u, Wt->rn), *dl = up_f64(lambda, Wt->cn);
  double *dout = (double *)amgd_alloc(Wt->nnz * 8 + 8);
  amgd_memset(dout, 0xff, Wt->nnz * 8 + 8);
  amgd_qapply(Wt, Q, qoff, Bt, du, dl, dout);
  amgd_sync();
  if (Wt->nnz) amgd_d2h(out, dout, Wt->nnz * 8);
  amgd_free(Q); amgd_free(qoff); amgd_free(du); amgd_free(dl); amgd_free(dout);
  dcsr_free(&Wt); dcsr_free(&A); dcsr_free(&Bt);
  return 0;
}
/* out (nnz(S) doubles) = S's values after amgd_lmop on the caller's S pattern (nf x nf),
   W_skel (nf x nc, values 1, 0 on the dirty entries), A (nf x nf) and u (nc); Wt, its map,
   kpos and the Q factors are formed as the setup forms them.  S's values start as a NaN
   pattern: amgd_lmop has to clear them itself. */
API int amgd_test_lmop(const hcsr *HS, const hcsr *HWskel, const hcsr *HA, const double *u, double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (HS->rn != HWskel->rn || HA->rn != HWskel->rn) return -2;
  dcsr *S = up(HS), *Wskel = up(HWskel), *A = up(HA);
  if (S->nnz) amgd_memset(S->a, 0xff, S->nnz * 8);
  uint64_t *perm = NULL, tot = 0, *qoff = NULL;
  dcsr *Wt = amgd_transpose(Wskel, &perm);
  uint32_t *kpos = amgd_lmop_kpos(Wt, perm);
  double *Q = amgd_qfactor(Wt, A, &qoff, &tot);
  double *du = up_f64(u, Wt->rn);
  const int rc = amgd_lmop(S, Wskel, kpos, Wt, Q, qoff, du);
  amgd_sync();
  if (S->nnz) amgd_d2h(out, S->a, S->nnz * 8);
  amgd_free(Q); amgd_free(qoff); amgd_free(du); amgd_free(kpos); amgd_free(perm);
  dcsr_free(&Wt); dcsr_free(&S); dcsr_free(&Wskel); dcsr_free(&A);
  return rc;
}

/* ---------------------------------------------------------------------------
 * V-cycle (amgd_vcycle.c, tests/test_gpu_solve.py): one level's up-sweep and one level's
 * restriction on host operands, with m and the row shapes chosen freely, and the switches.
 * --------------------------------------------------------------------------- */
extern int amgd_vc_level_run(const dcsr *Af, const dcsr *W, const dcsr *AfP, const double *D, uint32_t m,
                             double rho, double *x, double *b, double *c_out, int mode);
extern void amgd_vc_restrict_run(const dcsr *W, double *bF, double *bC, int fused);
extern void amgd_vc_stats_reset(void);
/* Af nf x nf, W and AfP nf x nc (columns 0..nc-1), D and bf nf, xc nc.  mode 0 composed,
   1 fused, 2 the one-workgroup tail kernel (nf + nc <= 1024, else -1).  Out: xf, bf, c (nf) */
API int amgd_test_vc_level(const hcsr *HAf, const hcsr *HW, const hcsr *HAfP, const double *D, uint32_t m,
                           double rho, const double *bf, const double *xc, int mode, double *xf_out,
                           double *bf_out, double *c_out) {
  if (amgd_rt_init(0) != 0) return -1;
  const uint32_t nf = HW->rn, nc = HW->cn;
  dcsr *Af = up(HAf), *W = up(HW), *AfP = up(HAfP);
  double *dD = up_f64(D, nf), *x = (double *)amgd_alloc(((size_t)nf + nc) * 8 + 8);
  double *b = (double *)amgd_alloc(((size_t)nf + nc) * 8 + 8), *c = (double *)amgd_alloc((size_t)nf * 8 + 8);
  amgd_memset(x, 0xff, (size_t)nf * 8);                 /* xf is written, never read first */
  amgd_memset(b, 0, ((size_t)nf + nc) * 8);
  if (nc) amgd_h2d(x + nf, xc, (size_t)nc * 8);
  if (nf) amgd_h2d(b, bf, (size_t)nf * 8);
  const int rc = amgd_vc_level_run(Af, W, AfP, dD, m, rho, x, b, c, mode);
  if (rc == 0 && nf) {
    amgd_d2h(xf_out, x, (size_t)nf * 8);
    amgd_d2h(bf_out, b, (size_t)nf * 8);
    amgd_d2h(c_out, c, (size_t)nf * 8);
  }
  amgd_free(dD); amgd_free(x); amgd_free(b); amgd_free(c);
  dcsr_free(&Af); dcsr_free(&W); dcsr_free(&AfP);
  return rc;
}
/* bC (nc, in / out) += W' bF (nf) */
API int amgd_test_vc_restrict(const hcsr *HW, const double *bF, double *bC, int fused) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *W = up(HW);
  double *dF = up_f64(bF, HW->rn), *dC = up_f64(bC, HW->cn);
  amgd_vc_restrict_run(W, dF, dC, fused);
  if (HW->cn) amgd_d2h(bC, dC, (size_t)HW->cn * 8);
  amgd_free(dF); amgd_free(dC);
  dcsr_free(&W);
  return 0;
}
/* K = 2 / 4 / 8 columns (amgd_solve.hip over the K-column policies), host blocks column-major: X K columns of
   nf + nc (xf out, xc in), B K columns of nf (bf in / out), C_out K columns of nf; family 0 by
   row shape, 1 the short-row kernels, 2 the long-row kernels */
extern int amgd_vc_level_run_n(const dcsr *Af, const dcsr *W, const dcsr *AfP, const double *D, uint32_t m,
                               double rho, double *X, double *B, double *C_out, int K, int family);
extern int amgd_vc_restrict_run_n(const dcsr *W, double *BF, double *BC, int K, int family);
API int amgd_test_vc_level_n(const hcsr *HAf, const hcsr *HW, const hcsr *HAfP, const double *D, uint32_t m,
                             double rho, double *X, double *B, double *C_out, int K, int family) {
  if (amgd_rt_init(0) != 0) return -1;
  if (K < 1 || K > 8) return -1;
  const uint32_t nf = HW->rn, nc = HW->cn;
  const size_t nx = ((size_t)nf + nc) * K, nb = (size_t)nf * K;
  dcsr *Af = up(HAf), *W = up(HW), *AfP = up(HAfP);
  double *dD = up_f64(D, nf), *x = up_f64(X, nx), *b = up_f64(B, nb), *c = (double *)amgd_alloc(nb * 8 + 8);
  const int rc = amgd_vc_level_run_n(Af, W, AfP, dD, m, rho, x, b, c, K, family);
  if (rc == 0) {
    amgd_d2h(X, x, nx * 8);
    if (nb) { amgd_d2h(B, b, nb * 8); amgd_d2h(C_out, c, nb * 8); }
  }
  amgd_free(dD); amgd_free(x); amgd_free(b); amgd_free(c);
  dcsr_free(&Af); dcsr_free(&W); dcsr_free(&AfP);
  return rc;
}
/* BC (K columns of nc, in / out) += W' BF (K columns of nf) */
API int amgd_test_vc_restrict_n(const hcsr *HW, const double *BF, double *BC, int K, int family) {
  if (amgd_rt_init(0) != 0) return -1;
  if (K < 1 || K > 8) return -1;
  dcsr *W = up(HW);
  double *dF = up_f64(BF, (size_t)HW->rn * K), *dC = up_f64(BC, (size_t)HW->cn * K);
  const int rc = amgd_vc_restrict_run_n(W, dF, dC, K, family);
  if (rc == 0 && HW->cn) amgd_d2h(BC, dC, (size_t)HW->cn * K * 8);
  amgd_free(dF); amgd_free(dC);
  dcsr_free(&W);
  return rc;
}
extern uint64_t amgd_vc_launches(void);
API uint64_t amgd_test_vc_launches(void) { return amgd_vc_launches(); }
API void amgd_test_vc_stats_reset(void) { amgd_vc_stats_reset(); }
/* event pairs queued on the library's timers and not read yet (a solve must not grow them) */
API uint64_t amgd_test_timer_pending(void) { return amgd_timer_pending(); }

/* ---------------------------------------------------------------------------
 * The partitioned V-cycle (amgd_vcycle.c, tests/test_gpu_part_solve.py): its switches, the
 * mapped restriction on host operands, and one halo exchange on its own.
 * --------------------------------------------------------------------------- */
extern void amgd_vc_restrict_map_run(const dcsr *Wt, const double *bF, double *b, const uint32_t *map, int mode);
extern void amgd_vc_halo_test(const dcsr *M, const uint32_t *split, uint32_t n, double *v);
/* b (nb, in / out): b[map[c]] += row c of Wt (rn rows, columns index bF) times bF; mode 0
   composed, 1 thread per row, 2 cooperative */
API int amgd_test_vc_restrict_map(const hcsr *HWt, const double *bF, double *b, uint32_t nb, const uint32_t *map,
                                  int mode) {
  if (amgd_rt_init(0) != 0) return -1;
  dcsr *Wt = up(HWt);
  double *dF = up_f64(bF, HWt->cn), *db = up_f64(b, nb);
  uint32_t *dm = (uint32_t *)amgd_alloc((size_t)HWt->rn * 4 + 8);
  if (HWt->rn) amgd_h2d(dm, map, (size_t)HWt->rn * 4);
  amgd_vc_restrict_map_run(Wt, dF, db, dm, mode);
  if (nb) amgd_d2h(b, db, (size_t)nb * 8);
  amgd_free(dF); amgd_free(db); amgd_free(dm);
  dcsr_free(&Wt);
  return 0;
}
/* Every rank passes the whole host matrix M, its row split and the split of the vector its
   columns index (np + 1 entries each), and v (M->cn entries, in / out): the rank keeps its row
   block, builds the halo list and runs one exchange on v */
API int amgd_test_vc_halo_xch(const hcsr *M, const uint32_t *rsplit, const uint32_t *vsplit, double *v) {
  if (amgd_rt_init(0) != 0) return -1;
  apart rp;
  fill_part(&rp, rsplit);
  dcsr *A = up_rows(M, &rp, 0);
  double *dv = up_f64(v, M->cn);
  amgd_vc_halo_test(A, vsplit, M->cn, dv);
  if (M->cn) amgd_d2h(v, dv, (size_t)M->cn * 8);
  amgd_free(dv);
  dcsr_free(&A);
  return 0;
}
struct amgd_hier;
extern int amgd_vc_plan_levels(const struct amgd_hier *h, uint64_t *out, int cap);
API int amgd_test_vc_plan_levels(const struct amgd_hier *h, uint64_t *out, int cap) {
  return amgd_vc_plan_levels(h, out, cap);
}

/* ---------------------------------------------------------------------------
 * Flexible GMRES (amgd_krylov.hip, tests/test_gpu_krylov.py): the multi-dot and the update on
 * a host basis block V (nb columns, column t at + t*ld, ld >= n; the padding is uploaded too
 * and must not be read) and a host w (n).
 * --------------------------------------------------------------------------- */
API int amgd_test_kry_tile(void) { return amgd_kry_tile(); }
/* out[t] = v_t . w, t < nb */
API int amgd_test_kry_mdot(const double *V, const double *w, uint64_t n, uint64_t ld, int nb, double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nb < 1 || ld < n || n < 1) return -1;
  double *dV = up_f64(V, (size_t)nb * ld), *dw = up_f64(w, n), *d = (double *)amgd_alloc((size_t)nb * 8 + 8);
  double *part = (double *)amgd_alloc((size_t)nb * (size_t)amgd_kry_grid(n) * 8 + 8);
  amgd_kry_mdot(dV, ld, dw, n, nb, part, d, NULL, NULL);
  amgd_d2h(out, d, (size_t)nb * 8);
  amgd_free(dV); amgd_free(dw); amgd_free(d); amgd_free(part);
  return 0;
}
/* w (n, in / out) = ((w - d_0 v_0) - d_1 v_1) - ...; nrm2_out (may be NULL): the kernel's sum of
   the new w's squares and its square root */
API int amgd_test_kry_update(const double *V, double *w, const double *d, uint64_t n, uint64_t ld, int nb,
                             double *nrm2_out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nb < 1 || ld < n || n < 1) return -1;
  double *dV = up_f64(V, (size_t)nb * ld), *dw = up_f64(w, n), *dd = up_f64(d, (size_t)nb);
  double *part = (double *)amgd_alloc((size_t)amgd_kry_grid(n) * 8 + 8), *nrm = (double *)amgd_alloc(16);
  amgd_kry_axpys(dw, dV, ld, dd, nb, n, 0, part, nrm2_out ? nrm : NULL, nrm2_out ? nrm + 1 : NULL);
  amgd_d2h(w, dw, n * 8);
  if (nrm2_out) amgd_d2h(nrm2_out, nrm, 16);
  amgd_free(dV); amgd_free(dw); amgd_free(dd); amgd_free(part); amgd_free(nrm);
  return 0;
}
/* ---- the flexible GMRES on a row-partitioned hierarchy: its pieces on host operands, every
   rank of the partitioned communicator making the same call (tests/part_krylov_worker.py) ---- */
extern void amgd_kry_mdot_ranks_run(const double *V, uint64_t ld, const double *w, uint64_t n, int nb, double *d);
extern void amgd_kry_norm_ranks_run(double *w, const double *V, uint64_t ld, const double *c, int nb, uint64_t n,
                                    double *nrm);
extern void amgd_vc_spmv_part_test(const dcsr *M, const uint32_t *split, uint32_t n, double *v, double *z);
/* out[t] = the ranks' sums v_t . w on their own rows (n of them here, n = 0 allowed) added in rank order */
API int amgd_test_kry_mdot_ranks(const double *V, const double *w, uint64_t n, uint64_t ld, int nb, double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nb < 1 || nb > 65 || ld < n || (ld & 1)) return -1;
  double *dV = up_f64(V, (size_t)nb * ld), *dw = up_f64(w, n), *d = (double *)amgd_alloc((size_t)nb * 8 + 8);
  amgd_kry_mdot_ranks_run(dV, ld, dw, n, nb, d);
  amgd_d2h(out, d, (size_t)nb * 8);
  amgd_free(dV); amgd_free(dw); amgd_free(d);
  return 0;
}
/* w (n, in / out) = ((w - d_0 v_0) - ...) on the own rows; nrm_out: the ranks' sums of the new
   w's squares added in rank order, and the square root */
API int amgd_test_kry_norm_ranks(const double *V, double *w, const double *d, uint64_t n, uint64_t ld, int nb,
                                 double *nrm_out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nb < 1 || nb > 65 || ld < n || (ld & 1)) return -1;
  double *dV = up_f64(V, (size_t)nb * ld), *dw = up_f64(w, n), *dd = up_f64(d, (size_t)nb);
  double *nrm = (double *)amgd_alloc(16 + 8);
  amgd_kry_norm_ranks_run(dw, dV, ld, dd, nb, n, nrm);
  if (n) amgd_d2h(w, dw, n * 8);
  amgd_d2h(nrm_out, nrm, 16);
  amgd_free(dV); amgd_free(dw); amgd_free(dd); amgd_free(nrm);
  return 0;
}
/* Every rank passes the whole host matrix M, its row split, the split of the vector its columns
   index and v (M->cn entries, valid on the own ones; in / out): the rank keeps its row block,
   fetches the entries its rows read and forms z (its rows of M v, rsplit[me+1] - rsplit[me]) */
API int amgd_test_kry_spmv_part(const hcsr *M, const uint32_t *rsplit, const uint32_t *vsplit, double *v, double *z) {
  if (amgd_rt_init(0) != 0) return -1;
  apart rp;
  fill_part(&rp, rsplit);
  dcsr *A = up_rows(M, &rp, 0);
  double *dv = up_f64(v, M->cn), *dz = (double *)amgd_alloc((size_t)A->rn * 8 + 8);
  amgd_vc_spmv_part_test(A, vsplit, M->cn, dv, dz);
  if (M->cn) amgd_d2h(v, dv, (size_t)M->cn * 8);
  if (A->rn) amgd_d2h(z, dz, (size_t)A->rn * 8);
  amgd_free(dv); amgd_free(dz);
  dcsr_free(&A);
  return 0;
}
/* the floor of an inner iteration (tools/solve_bench.py --krylov): one cycle and one level-0
   product on the workspace of an earlier amgd_krylov_device call, on the Krylov timer */
struct amgd_hier;
extern int amgd_kry_floor(struct amgd_hier *h, double *dx, const double *db);
API int amgd_test_kry_floor(struct amgd_hier *h, double *dx, const double *db) { return amgd_kry_floor(h, dx, db); }

/* ---------------------------------------------------------------------------
 * Flexible GMRES on several right-hand sides (amgd_krylov_device_n,
 * tests/test_gpu_krylov_mrhs.py): the slot count, the K-column level-0 product and the
 * multi-column orthogonalisation kernels on host operands.
 * --------------------------------------------------------------------------- */
extern void amgd_kry_products_run(const dcsr *A, int K, int family, const double *const *x, double *const *z,
                                  double alpha, const double *const *y, double beta);
/* Z_j = alpha*Y_j + beta*(A X_j), j < K: X is K columns of cn doubles, Y (may be NULL) and Z K
   columns of rn, contiguous on the host.  On the device every column is an allocation of its
   own, and where bit j of shift is set column j of X, Y and Z starts one double into it (a
   pointer aligned to 8 bytes only).  A matrix with an outlier row goes column by column through
   amgd_spmv (route counter kry_n_comp) */
API int amgd_test_kry_spmv_n(const hcsr *HA, const double *X, const double *Y, double *Z, int K, double alpha,
                             double beta, int family, unsigned shift) {
  if (amgd_rt_init(0) != 0) return -1;
  if (K != 2 && K != 4 && K != 8) return -1;
  dcsr *A = up(HA);
  const size_t rn = HA->rn, cn = HA->cn;
  double *bx[8], *by[8], *bz[8], *z[8];
  const double *x[8], *y[8];
  for (int j = 0; j < K; j++) {
    const size_t s = (shift >> j) & 1;
    bx[j] = (double *)amgd_alloc((cn + 2) * 8);
    by[j] = (double *)amgd_alloc((rn + 2) * 8);
    bz[j] = (double *)amgd_alloc((rn + 2) * 8);
    if (cn) amgd_h2d(bx[j] + s, X + j * cn, cn * 8);
    if (Y && rn) amgd_h2d(by[j] + s, Y + j * rn, rn * 8);
    x[j] = bx[j] + s;
    y[j] = by[j] + s;
    z[j] = bz[j] + s;
  }
  amgd_kry_products_run(A, K, family, x, z, alpha, Y ? y : NULL, beta);
  for (int j = 0; j < K; j++) {
    if (rn) amgd_d2h(Z + j * rn, z[j], rn * 8);
    amgd_free(bx[j]); amgd_free(by[j]); amgd_free(bz[j]);
  }
  dcsr_free(&A);
  return 0;
}
/* amgd_test_kry_mdot for nc <= 8 columns in one launch: column q has nbs[q] basis vectors (its
   block of nbs[q]*ld doubles follows column q - 1's in V) and its own w (w + q*n); out: the
   dots, column after column */
API int amgd_test_kry_mdot_n(const double *V, const double *w, uint64_t n, uint64_t ld, int nc, const int *nbs,
                             double *out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nc < 1 || nc > 8 || ld < n || n < 1) return -1;
  amgd_kry_col C[8];
  memset(C, 0, sizeof C);
  size_t at = 0;
  for (int q = 0; q < nc; q++) {
    const int nb = nbs[q];
    if (nb < 1) return -1;
    C[q].V = up_f64(V + at, (size_t)nb * ld);
    C[q].w = up_f64(w + (size_t)q * n, n);
    C[q].nb = nb;
    C[q].d = (double *)amgd_alloc((size_t)nb * 8 + 8);
    C[q].part = (double *)amgd_alloc((size_t)nb * (size_t)amgd_kry_grid(n) * 8 + 8);
    at += (size_t)nb * ld;
  }
  amgd_kry_mdot_n(C, nc, ld, n);
  at = 0;
  for (int q = 0; q < nc; q++) {
    amgd_d2h(out + at, C[q].d, (size_t)C[q].nb * 8);
    at += (size_t)C[q].nb;
    amgd_free((void *)C[q].V); amgd_free(C[q].w); amgd_free(C[q].d); amgd_free(C[q].part);
  }
  return 0;
}
/* amgd_test_kry_update for nc <= 8 columns in one launch: V and nbs as above, w (nc*n, in / out),
   d the coefficients column after column; nrm2_out (may be NULL): per column the sum of the new
   w's squares and its square root */
API int amgd_test_kry_update_n(const double *V, double *w, const double *d, uint64_t n, uint64_t ld, int nc,
                               const int *nbs, double *nrm2_out) {
  if (amgd_rt_init(0) != 0) return -1;
  if (nc < 1 || nc > 8 || ld < n || n < 1) return -1;
  amgd_kry_col C[8];
  memset(C, 0, sizeof C);
  size_t at = 0, dat = 0;
  for (int q = 0; q < nc; q++) {
    const int nb = nbs[q];
    if (nb < 1) return -1;
    C[q].V = up_f64(V + at, (size_t)nb * ld);
    C[q].w = up_f64(w + (size_t)q * n, n);
    C[q].nb = nb;
    C[q].d = up_f64(d + dat, (size_t)nb);
    C[q].part = (double *)amgd_alloc((size_t)amgd_kry_grid(n) * 8 + 8);
    if (nrm2_out) {
      C[q].nrm2 = (double *)amgd_alloc(16);
      C[q].root = C[q].nrm2 + 1;
    }
    at += (size_t)nb * ld;
    dat += (size_t)nb;
  }
  amgd_kry_axpys_n(C, nc, ld, n);
  for (int q = 0; q < nc; q++) {
    amgd_d2h(w + (size_t)q * n, C[q].w, n * 8);
    if (nrm2_out) { amgd_d2h(nrm2_out + 2 * q, C[q].nrm2, 16); amgd_free(C[q].nrm2); }
    amgd_free((void *)C[q].V); amgd_free(C[q].w); amgd_free(C[q].d); amgd_free(C[q].part);
  }
  return 0;
}
/* the floor of a lock-step step of K columns (tools/solve_bench.py --krylov --nrhs): K cycles and
   K level-0 products in a step's groups, on the multi-RHS Krylov timer */
extern int amgd_kry_floor_n(struct amgd_hier *h, int K);
API int amgd_test_kry_floor_n(struct amgd_hier *h, int K) { return amgd_kry_floor_n(h, K); }
