// amgd_solve.hip -- the V-cycle's own kernels (driver: amgd_vcycle.c; contract: DESIGN.md
// "Solve").  Every product is the reference's apply_M row sum (amg_tools.c:77-99): the
// products a_ij * x_j added left to right from +0, no FMA (-ffp-contract=off), then
// alpha*y + beta*t with alpha, beta = +-1 -- so each kernel here gives the bits the composed
// path (amgd_spmv + the vector kernels) gives, which the tests hold it to.
//
// A level has three operations -- restriction, prolongation, one Chebyshev step -- and each is
// ONE kernel template over a row-sum policy (amgd_vc_dev.h): one vector or K = 2, 4, 8
// interleaved ones, short rows (a block per 256 rows) or long rows (a wavefront per row group).
// The pointwise arithmetic of all of them, of the one-workgroup coarse tail (which runs the
// deepest levels in a single launch) and of the composed path's update kernel (amgd_vec.hip) is
// the update functions of amgd_vc_dev.h and nothing else, so column j of a group comes out bit
// for bit as the single-vector cycle gives it, whatever K and whichever policy.  A matrix with
// an outlier row takes the composed path (amgd_vcycle.c routes and counts: vc_thr / vc_wave /
// vc_comp / vc_tail; for K columns the driver runs that level column by column).
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"
#include "amgd_vc_dev.h"

// ordered row sum of one CSR row against x, one thread alone (the coarse tail)
__device__ __forceinline__ double vc_row(const uint64_t *ro, const uint32_t *col, const double *a,
                                         const double *x, uint64_t i) {
  double t = 0.0;
  const uint64_t k1 = ro[i + 1];
  for (uint64_t k = ro[i]; k < k1; k++) t += a[k] * x[col[k]];
  return t;
}

__global__ void k_vc_remap(const uint32_t *col, uint64_t nnz, const uint32_t *pos, uint32_t off,
                           uint32_t *out) {
  GRID_STRIDE(k, nnz) out[k] = pos[col[k]] - off;
}
extern "C" void amgd_vc_remap_cols(const uint32_t *col, uint64_t nnz, const uint32_t *pos_next,
                                   uint32_t off_next, uint32_t *out) {
  if (nnz) k_vc_remap<<<grid_for(nnz), 256, 0, amgd_s()>>>(col, nnz, pos_next, off_next, out);
  KCHECK();
}
__global__ void k_vc_scatter(double *b, const double *db, const uint32_t *pos, uint64_t n) {
  GRID_STRIDE(i, n) b[pos[i]] = db[i];
}
extern "C" void amgd_vc_scatter(double *b, const double *db, const uint32_t *pos, uint64_t n) {
  if (n) k_vc_scatter<<<grid_for(n), 256, 0, amgd_s()>>>(b, db, pos, n);
  KCHECK();
}
__global__ void k_vc_gather(double *dx, const double *x, const uint32_t *pos, uint64_t n, int sub,
                            double avg) {
  GRID_STRIDE(i, n) {
    const double v = x[pos[i]];
    dx[i] = sub ? v - avg : v;
  }
}
extern "C" void amgd_vc_gather(double *dx, const double *x, const uint32_t *pos, uint64_t n, int sub,
                               double avg) {
  if (n) k_vc_gather<<<grid_for(n), 256, 0, amgd_s()>>>(dx, x, pos, n, sub, avg);
  KCHECK();
}
// the composed restriction's second half on a rank's own C rows
__global__ void k_vc_add_map(double *b, const uint32_t *map, const double *t, uint64_t n) {
  GRID_STRIDE(c, n) {
    const uint32_t q = map[c];
    b[q] = vc_add(b[q], t[c]);
  }
}
extern "C" void amgd_vc_add_map(double *b, const uint32_t *map, const double *t, uint64_t n) {
  if (n) k_vc_add_map<<<grid_for(n), 256, 0, amgd_s()>>>(b, map, t, n);
  KCHECK();
}
// halo exchange of the partitioned cycle: the entries a peer asked for into one send buffer,
// the entries received to their places
__global__ void k_vc_pack(double *buf, const double *v, const uint32_t *idx, uint64_t n) {
  GRID_STRIDE(k, n) buf[k] = v[idx[k]];
}
extern "C" void amgd_vc_pack(double *buf, const double *v, const uint32_t *idx, uint64_t n) {
  if (n) k_vc_pack<<<grid_for(n), 256, 0, amgd_s()>>>(buf, v, idx, n);
  KCHECK();
}
__global__ void k_vc_unpack(double *v, const uint32_t *idx, const double *buf, uint64_t n) {
  GRID_STRIDE(k, n) v[idx[k]] = buf[k];
}
extern "C" void amgd_vc_unpack(double *v, const uint32_t *idx, const double *buf, uint64_t n) {
  if (n) k_vc_unpack<<<grid_for(n), 256, 0, amgd_s()>>>(v, idx, buf, n);
  KCHECK();
}
// crs_solve on several ranks: the ranks' partial sums of b added in rank order from +0
__global__ void k_vc_rank_sum(double *out, const double *segs, int nr, uint64_t n) {
  GRID_STRIDE(i, n) {
    double t = 0.0;
    for (int r = 0; r < nr; r++) t += segs[(uint64_t)r * n + i];
    out[i] = t;
  }
}
extern "C" void amgd_vc_rank_sum(double *out, const double *segs, int nr, uint64_t n) {
  if (n) k_vc_rank_sum<<<grid_for(n), 256, 0, amgd_s()>>>(out, segs, nr, n);
  KCHECK();
}

// ---------------------------------------------------------------------------
// The three operations of a level.  The vectors of K interleaved columns are indexed by the
// finishing thread's element index e, D by its row i.
// ---------------------------------------------------------------------------
// b_{l+1} = 1*b_{l+1} + 1*(W' b_l[F]) (amg.c:125-126), in place on the tail of the flat b: row c
// of Wt reads the F slice only and writes position c of the coarse slice b alone.  MAP (one
// vector, a rank's own C rows in the partitioned cycle): row c writes position map[c] of the
// flat b -- the own C points are not contiguous in positions
template <class P, bool MAP>
__global__ __launch_bounds__(256) void k_vc_restrict(const uint64_t *ro, const uint32_t *col, const double *a,
                                                     uint32_t nc, const double *bF, double *b,
                                                     const uint32_t *map) {
  __shared__ typename P::Shared S;
  for (uint64_t g = P::first(); g < nc; g += P::stride()) {
    const VecK<P::OWN> t = P::rows(S, ro, col, a, bF, g, nc);
    if (P::owns(g, nc)) {
      const uint64_t e = MAP ? map[P::row(g)] : P::elem(g);
      VecK<P::OWN> v = ldk<P::OWN>(b + e);
#pragma unroll
      for (int j = 0; j < P::OWN; j++) v.v[j] = vc_add(v.v[j], t.v[j]);
      stk<P::OWN>(b + e, v);
    }
  }
}

// per F row: xf = W xc; bf = b - AfP xc; c = D.*bf; m == 1: xf += c (amg.c:142-146, :166):
// the row of W and the row of AfP against the same xc in one launch
template <class P>
__global__ __launch_bounds__(256) void k_vc_prolong(const uint64_t *wro, const uint32_t *wcol, const double *wa,
                                                    const uint64_t *pro, const uint32_t *pcol, const double *pa,
                                                    const double *D, uint32_t nf, const double *xc, double *xf,
                                                    double *bf, double *c, int add) {
  __shared__ typename P::Shared S;
  for (uint64_t g = P::first(); g < nf; g += P::stride()) {
    const VecK<P::OWN> xw = P::rows(S, wro, wcol, wa, xc, g, nf);
    const VecK<P::OWN> tp = P::rows(S, pro, pcol, pa, xc, g, nf);
    if (P::owns(g, nf)) {
      const uint64_t e = P::elem(g);
      const double d = D[P::row(g)];
      VecK<P::OWN> bv = ldk<P::OWN>(bf + e), cv, xv;
#pragma unroll
      for (int j = 0; j < P::OWN; j++) {
        const VcPro o = vc_prolong(bv.v[j], tp.v[j], d, xw.v[j], add);
        bv.v[j] = o.bb;
        cv.v[j] = o.cc;
        xv.v[j] = o.xf;
      }
      stk<P::OWN>(bf + e, bv);
      stk<P::OWN>(c + e, cv);
      stk<P::OWN>(xf + e, xv);
    }
  }
}

// one Chebyshev step in one pass over Af, no r vector: row i reads c at its columns and
// writes index i of the other buffer only (amg.c:152-155, :161-164; the last step adds
// into xf, amg.c:166).  cg: the vector the row sums gather from (Af's columns index it); c, cn,
// bf, D, xf: the rows' own entries.  One GPU: cg == c.  A rank's row block: cg the whole c, the
// rest offset to its rows
template <class P>
__global__ __launch_bounds__(256) void k_vc_cheb(const uint64_t *ro, const uint32_t *col, const double *a,
                                                 const double *D, uint32_t nf, const double *bf, const double *cg,
                                                 const double *c, double *cn, double beta, double gamma,
                                                 int has_prev, double *xf) {
  __shared__ typename P::Shared S;
  if (P::Cols > 1) cg = c;                   // K columns: cg == c (amgd_vc_cheb refuses anything else)
  for (uint64_t g = P::first(); g < nf; g += P::stride()) {
    const VecK<P::OWN> t = P::rows(S, ro, col, a, cg, g, nf);
    if (P::owns(g, nf)) {
      const uint64_t e = P::elem(g);
      const double d = D[P::row(g)];
      if constexpr (P::OWN == 1) {           // a single value: each operand read where the update uses it
        const double v = vc_cheb(bf[e], t.v[0], c[e], d, beta, gamma, has_prev, cn + e);
        cn[e] = v;
        if (xf) xf[e] = vc_add(xf[e], v);
      } else {                               // a K-wide piece: all reads in flight together
        const VecK<P::OWN> bv = ldk<P::OWN>(bf + e), cv = ldk<P::OWN>(c + e);
        VecK<P::OWN> nv, xv;
        if (has_prev) nv = ldk<P::OWN>(cn + e);
        if (xf) xv = ldk<P::OWN>(xf + e);
#pragma unroll
        for (int j = 0; j < P::OWN; j++) {
          const double v = vc_cheb(bv.v[j], t.v[j], cv.v[j], d, beta, gamma, has_prev, &nv.v[j]);
          nv.v[j] = v;
          if (xf) xv.v[j] = vc_add(xv.v[j], v);
        }
        stk<P::OWN>(cn + e, nv);
        if (xf) stk<P::OWN>(xf + e, xv);
      }
    }
  }
}

// The coarse tail: the deepest levels, whose flat slices together hold at most 1024
// positions, in ONE workgroup -- restriction down through them, the bottom solve, the
// up-sweep -- one thread per row and a block barrier between phases, instead of four to
// seven launches per level.  Level l's slices: F at [off, off + nf), coarse at
// [off + nf, N).  Same row sums, the same update functions and the same scalar sequence
// (beta / gamma from the host) as the per-level kernels.
__global__ __launch_bounds__(1024) void k_vc_tail(const amgd_vc_tlev *lv, int nl, double *b, double *x,
                                                  double *c0, double *c1, uint32_t N, double dbot,
                                                  int up_only) {
  const uint32_t t = threadIdx.x;
  if (!up_only) {
    for (int l = 0; l < nl; l++) {
      const amgd_vc_tlev *L = &lv[l];
      if (t < L->nc) {
        double *bC = b + L->off + L->nf;
        bC[t] = vc_add(bC[t], vc_row(L->wt_ro, L->wt_col, L->wt_a, b + L->off, t));
      }
      __syncthreads();
    }
    if (t == 0) x[N - 1] = dbot * b[N - 1];
    __syncthreads();
  }
  for (int l = nl - 1; l >= 0; l--) {
    const amgd_vc_tlev *L = &lv[l];
    double *xf = x + L->off, *bf = b + L->off;
    const double *xc = xf + L->nf;
    double *c = c0, *cn = c1;
    if (t < L->nf) {
      const double xw = vc_row(L->w_ro, L->w_col, L->w_a, xc, t);
      const VcPro o = vc_prolong(bf[t], vc_row(L->p_ro, L->p_col, L->p_a, xc, t), L->D[t], xw, L->steps == 0);
      bf[t] = o.bb;
      c[t] = o.cc;
      xf[t] = o.xf;
    }
    __syncthreads();
    for (uint32_t k = 0; k < L->steps; k++) {
      if (t < L->nf) {
        const double v = vc_cheb(bf[t], vc_row(L->af_ro, L->af_col, L->af_a, c, t), c[t], L->D[t], L->beta[k],
                                 L->gamma[k], k > 0, cn + t);
        cn[t] = v;
        if (k + 1 == L->steps) xf[t] = vc_add(xf[t], v);
      }
      __syncthreads();
      double *s = c; c = cn; cn = s;
    }
  }
}
extern "C" void amgd_vc_tail(const amgd_vc_tlev *lv, int nl, double *b, double *x, double *c0, double *c1,
                             uint32_t N, double dbot, int up_only) {
  k_vc_tail<<<1, 1024, 0, amgd_s()>>>(lv, nl, b, x, c0, c1, N, dbot, up_only);
  KCHECK();
}

// ---------------------------------------------------------------------------
// The entry points: fam 0 short rows, 1 long rows; K == 1 one vector, else 2 / 4 / 8 interleaved
// ---------------------------------------------------------------------------
static inline int vc_rw(uint64_t n) {
  const int64_t rw = amgd_knob(AMGD_K_VC_RW);   // tests: 4 / 16 / 64 forces the shape, else by row count
  if (rw == 4 || rw == 16 || rw == 64) return (int)rw;
  return n >= (1ull << 22) ? 64 : n >= (1ull << 16) ? 16 : 4;
}
// go(P{}) for the policy P that (fam, K, n) names
template <class F> static void vc_with_policy(int fam, int K, uint32_t n, F &&go) {
  const int rw = K == 1 && fam ? vc_rw(n) : 0;
  if (K == 1 && !fam) go(VcBlock{});
  else if (rw == 64) go(VcCoop<64, 16>{});
  else if (rw == 16) go(VcCoop<16, 16>{});
  else if (rw == 4) go(VcCoop<4, 8>{});
  else if (K == 8) fam ? go(VnCoop<8>{}) : go(VnBlock<8>{});
  else if (K == 4) fam ? go(VnCoop<4>{}) : go(VnBlock<4>{});
  else fam ? go(VnCoop<2>{}) : go(VnBlock<2>{});
  KCHECK();
}
static inline bool vc_k_ok(int K) { return K == 1 || K == 2 || K == 4 || K == 8; }
extern "C" void amgd_vc_restrict(int fam, int K, const dcsr *Wt, const double *bF, double *b,
                                 const uint32_t *map) {
  if (!Wt->rn || !vc_k_ok(K)) return;
  if (map && K != 1) {
    amgd_set_error("amgd_vc_restrict: the indexed write exists for one vector only");
    return;
  }
  vc_with_policy(fam, K, Wt->rn, [&](auto p) {
    using P = decltype(p);
    const int g = P::grid(Wt->rn);
    if constexpr (P::Cols == 1) {
      if (map) {
        k_vc_restrict<P, true><<<g, 256, 0, amgd_s()>>>(Wt->ro, Wt->col, Wt->a, Wt->rn, bF, b, map);
        return;
      }
    }
    k_vc_restrict<P, false><<<g, 256, 0, amgd_s()>>>(Wt->ro, Wt->col, Wt->a, Wt->rn, bF, b, map);
  });
}
extern "C" void amgd_vc_prolong(int fam, int K, const dcsr *W, const dcsr *AfP, const double *D, const double *xc,
                                double *xf, double *bf, double *c, int add) {
  if (!W->rn || !vc_k_ok(K)) return;
  vc_with_policy(fam, K, W->rn, [&](auto p) {
    using P = decltype(p);
    k_vc_prolong<P><<<P::grid(W->rn), 256, 0, amgd_s()>>>(W->ro, W->col, W->a, AfP->ro, AfP->col, AfP->a, D, W->rn,
                                                           xc, xf, bf, c, add);
  });
}
extern "C" void amgd_vc_cheb(int fam, int K, const dcsr *Af, const double *D, const double *bf, const double *cg,
                             const double *c, double *cn, double beta, double gamma, int has_prev, double *xf) {
  if (!Af->rn || !vc_k_ok(K)) return;
  if (K != 1 && cg != c) {
    amgd_set_error("amgd_vc_cheb: K columns gather from their own c (cg == c)");
    return;
  }
  vc_with_policy(fam, K, Af->rn, [&](auto p) {
    using P = decltype(p);
    k_vc_cheb<P><<<P::grid(Af->rn), 256, 0, amgd_s()>>>(Af->ro, Af->col, Af->a, D, Af->rn, bf, cg, c, cn, beta,
                                                         gamma, has_prev, xf);
  });
}
