// amgd_solve_mrhs.hip -- the V-cycle's kernels for a group of K = 2, 4 or 8 right-hand sides
// (driver: amgd_vcycle.c, "several right-hand sides"; contract: DESIGN.md "Solve").
//
// Layout: the K vectors of a group are interleaved, element (position q, column j) at q*K + j,
// so a row's thread loads each (value, column) pair ONCE for K products and gathers the K
// operands of an entry with one contiguous 8K-byte read.  Every (row, column) sum is the
// single-vector kernels' sum (amgd_solve.hip): the products a_ik * x_kj added left to right
// over the row's entries from +0, no FMA (-ffp-contract=off), and the pointwise updates are
// those kernels' expressions verbatim -- column j of a group comes out bit for bit as the
// single-vector cycle gives it, whatever K and whichever kernel family.
//
// Two families, as for one vector: short rows (a block owns 256 consecutive rows and walks
// their entry range in chunks) and long rows (a wavefront owns 64 / K rows and walks them in
// rounds of 16 entries per row).  A matrix with an outlier row has no form here: the driver
// runs that level's operation column by column through the single-vector code.
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"

#include "amgd_mrhs_dev.h"


// ---------------------------------------------------------------------------
// Short rows.  vc_block_rows (amgd_solve.hip) stages the chunk's PRODUCTS in LDS, which would
// take K times its 32 KB here; this form stages the chunk's (value, column) pairs instead
// (12 B per entry, 24 KB a block: no more LDS than one vector takes) and the row's thread
// forms its K products from one contiguous read of x[col*K .. col*K + K).  Chunks in order
// and entries in order inside a chunk: the ordered sum per column, whatever the row lengths.
// ---------------------------------------------------------------------------

template <int K>
__global__ __launch_bounds__(256) void k_vcn_restrict(const uint64_t *ro, const uint32_t *col, const double *a,
                                                      uint32_t nc, const double *bF, double *bC) {
  __shared__ double sa[VN_CH];
  __shared__ uint32_t sc[VN_CH];
  VN_BLOCK_LOOP(nc) {
    const uint64_t r1 = min((uint64_t)nc, r0 + VN_ROWS), c = r0 + threadIdx.x;
    const bool own = c < r1;
    const VecK<K> t = vn_block_rows<K>(sa, sc, ro, col, a, bF, r0, r1, c, own);
    if (own) {
      VecK<K> v = ldk<K>(bC + c * K);
#pragma unroll
      for (int j = 0; j < K; j++) v.v[j] = v.v[j] + t.v[j];
      stk<K>(bC + c * K, v);
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_vcn_prolong(const uint64_t *wro, const uint32_t *wcol, const double *wa,
                                                     const uint64_t *pro, const uint32_t *pcol, const double *pa,
                                                     const double *D, uint32_t nf, const double *xc, double *xf,
                                                     double *bf, double *c, int add) {
  __shared__ double sa[VN_CH];
  __shared__ uint32_t sc[VN_CH];
  VN_BLOCK_LOOP(nf) {
    const uint64_t r1 = min((uint64_t)nf, r0 + VN_ROWS), i = r0 + threadIdx.x;
    const bool own = i < r1;
    const VecK<K> xw = vn_block_rows<K>(sa, sc, wro, wcol, wa, xc, r0, r1, i, own);
    const VecK<K> tp = vn_block_rows<K>(sa, sc, pro, pcol, pa, xc, r0, r1, i, own);
    if (own) {
      const double d = D[i];
      VecK<K> bv = ldk<K>(bf + i * K), cv, xv;
#pragma unroll
      for (int j = 0; j < K; j++) {
        const double bb = bv.v[j] - tp.v[j];
        const double cc = d * bb;
        bv.v[j] = bb;
        cv.v[j] = cc;
        xv.v[j] = add ? xw.v[j] + cc : xw.v[j];
      }
      stk<K>(bf + i * K, bv);
      stk<K>(c + i * K, cv);
      stk<K>(xf + i * K, xv);
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_vcn_cheb(const uint64_t *ro, const uint32_t *col, const double *a,
                                                  const double *D, uint32_t nf, const double *bf, const double *c,
                                                  double *cn, double beta, double gamma, int has_prev, double *xf) {
  __shared__ double sa[VN_CH];
  __shared__ uint32_t sc[VN_CH];
  VN_BLOCK_LOOP(nf) {
    const uint64_t r1 = min((uint64_t)nf, r0 + VN_ROWS), i = r0 + threadIdx.x;
    const bool own = i < r1;
    const VecK<K> t = vn_block_rows<K>(sa, sc, ro, col, a, c, r0, r1, i, own);
    if (own) {
      const double d = D[i];
      const VecK<K> bv = ldk<K>(bf + i * K), cv = ldk<K>(c + i * K);
      VecK<K> nv, xv;
      if (has_prev) nv = ldk<K>(cn + i * K);
      if (xf) xv = ldk<K>(xf + i * K);
#pragma unroll
      for (int j = 0; j < K; j++) {
        const double r = bv.v[j] - t.v[j];
        double v = beta * (cv.v[j] + d * r);
        if (has_prev) v = v - gamma * nv.v[j];
        nv.v[j] = v;
        if (xf) xv.v[j] = xv.v[j] + v;
      }
      stk<K>(cn + i * K, nv);
      if (xf) stk<K>(xf + i * K, xv);
    }
  }
}

// ---------------------------------------------------------------------------
// Long rows, after VcTile (amgd_solve.hip): a wavefront owns RW = 64 / K rows and walks them in
// rounds of SEG = 16 entries per row.  A round's 64 * SEG / K (value, column) pairs are loaded
// coalesced, SEG / K per lane, all loads in flight together; each is multiplied with its K operands, gathered by one
// 8K-byte read, and the K products staged in an LDS tile.  Then lane r*K + j adds column j
// of row r's segment left to right: the ordered adds run on all 64 lanes, one per (row,
// column) pair, where the single-vector form has RW lanes adding and the rest idle.  The
// tile is 64 * 17 * 8 B a wavefront whatever K (the single-vector form's size at RW = 64);
// a row is padded by one entry slot, so the adding lanes of a 32-lane group read 32 distinct
// banks.  A row of any length is walked in rounds.  Lane r*K + j returns the sum of row
// rb + r, column j: its flat index rb*K + lane is contiguous over the wavefront.
// ---------------------------------------------------------------------------

template <int K>
__global__ __launch_bounds__(256) void k_vcn_restrict_wave(const uint64_t *ro, const uint32_t *col,
                                                           const double *a, uint32_t nc, const double *bF,
                                                           double *bC) {
  __shared__ VnTile<K> T;
  const int lane = threadIdx.x & 63;
  VN_WAVE_LOOP(nc) {
    const double t = vn_coop_rows<K>(T, ro, col, a, bF, rb, nc);
    if (rb + lane / K < nc) {
      const uint64_t e = rb * K + lane;
      bC[e] = bC[e] + t;
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_vcn_prolong_wave(const uint64_t *wro, const uint32_t *wcol,
                                                          const double *wa, const uint64_t *pro,
                                                          const uint32_t *pcol, const double *pa, const double *D,
                                                          uint32_t nf, const double *xc, double *xf, double *bf,
                                                          double *c, int add) {
  __shared__ VnTile<K> T;
  const int lane = threadIdx.x & 63;
  VN_WAVE_LOOP(nf) {
    const double xw = vn_coop_rows<K>(T, wro, wcol, wa, xc, rb, nf);
    const double tp = vn_coop_rows<K>(T, pro, pcol, pa, xc, rb, nf);
    const uint64_t i = rb + lane / K;
    if (i < nf) {
      const uint64_t e = rb * K + lane;
      const double bb = bf[e] - tp;
      const double cc = D[i] * bb;
      bf[e] = bb;
      c[e] = cc;
      xf[e] = add ? xw + cc : xw;
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void k_vcn_cheb_wave(const uint64_t *ro, const uint32_t *col, const double *a,
                                                       const double *D, uint32_t nf, const double *bf,
                                                       const double *c, double *cn, double beta, double gamma,
                                                       int has_prev, double *xf) {
  __shared__ VnTile<K> T;
  const int lane = threadIdx.x & 63;
  VN_WAVE_LOOP(nf) {
    const double t = vn_coop_rows<K>(T, ro, col, a, c, rb, nf);
    const uint64_t i = rb + lane / K;
    if (i < nf) {
      const uint64_t e = rb * K + lane;
      const double r = bf[e] - t;
      double v = beta * (c[e] + D[i] * r);
      if (has_prev) v = v - gamma * cn[e];
      cn[e] = v;
      if (xf) xf[e] = xf[e] + v;
    }
  }
}

// ---------------------------------------------------------------------------
// In and out of the interleaved level-ordered layout, the bottom solve, one column out.
// pos NULL: the identity (the level hooks).
// ---------------------------------------------------------------------------
struct VnAvg { double v[8]; };
// The columns come as a by-value table of pointers (amgd.h: a strided block and the lock-step
// Krylov solver's unequally strided columns alike).  A thread owns position i of every column:
// pos[i] is read once, the table is indexed by the unrolled j only (scalar reads, never a
// per-lane one), the K column loads are in flight together and the K values of a position are
// one aligned 8K-byte piece of the interleaved vector.
template <int K>
__global__ void k_vc_scatter_p(double *b, amgd_cptr8 in, const uint32_t *pos, uint64_t n) {
  GRID_STRIDE(i, n) {
    VecK<K> v;
#pragma unroll
    for (int j = 0; j < K; j++) v.v[j] = in.p[j][i];
    stk<K>(b + (pos ? pos[i] : i) * K, v);
  }
}
template <int K>
__global__ void k_vc_gather_p(amgd_ptr8 out, const double *x, const uint32_t *pos, uint64_t n, int sub, VnAvg avg) {
  GRID_STRIDE(i, n) {
    const VecK<K> v = ldk<K>(x + (pos ? pos[i] : i) * K);
#pragma unroll
    for (int j = 0; j < K; j++) out.p[j][i] = sub ? v.v[j] - avg.v[j] : v.v[j];
  }
}
extern "C" void amgd_vcn_scatter(double *b, const amgd_cptr8 *in, const uint32_t *pos, uint64_t n, int K) {
  if (!n) return;
  const int g = grid_for(n);
  if (K == 8) k_vc_scatter_p<8><<<g, 256, 0, amgd_s()>>>(b, *in, pos, n);
  else if (K == 4) k_vc_scatter_p<4><<<g, 256, 0, amgd_s()>>>(b, *in, pos, n);
  else if (K == 2) k_vc_scatter_p<2><<<g, 256, 0, amgd_s()>>>(b, *in, pos, n);
  KCHECK();
}
extern "C" void amgd_vcn_gather(const amgd_ptr8 *out, const double *x, const uint32_t *pos, uint64_t n, int K,
                                int sub, const double *avg) {
  if (!n) return;
  VnAvg A;
  for (int j = 0; j < 8; j++) A.v[j] = avg && j < K ? avg[j] : 0.0;
  const int g = grid_for(n);
  if (K == 8) k_vc_gather_p<8><<<g, 256, 0, amgd_s()>>>(*out, x, pos, n, sub, A);
  else if (K == 4) k_vc_gather_p<4><<<g, 256, 0, amgd_s()>>>(*out, x, pos, n, sub, A);
  else if (K == 2) k_vc_gather_p<2><<<g, 256, 0, amgd_s()>>>(*out, x, pos, n, sub, A);
  KCHECK();
}
__global__ void k_vc_bottom_n(double *x, const double *b, double dbot, int K) {
  const int j = threadIdx.x;
  if (j < K) x[j] = dbot * b[j];
}
__global__ void k_vc_col_n(double *out, const double *x, uint64_t n, int K, int j) {
  GRID_STRIDE(q, n) out[q] = x[q * K + j];
}
__global__ void k_vc_putcol_n(double *x, const double *in, uint64_t n, int K, int j) {
  GRID_STRIDE(q, n) x[q * K + j] = in[q];
}
extern "C" void amgd_vcn_putcol(double *x, const double *in, uint64_t n, int K, int j) {
  if (n) k_vc_putcol_n<<<grid_for(n), 256, 0, amgd_s()>>>(x, in, n, K, j);
  KCHECK();
}
extern "C" void amgd_vcn_bottom(double *x, const double *b, double dbot, int K) {
  k_vc_bottom_n<<<1, 64, 0, amgd_s()>>>(x, b, dbot, K);
  KCHECK();
}
extern "C" void amgd_vcn_col(double *out, const double *x, uint64_t n, int K, int j) {
  if (n) k_vc_col_n<<<grid_for(n), 256, 0, amgd_s()>>>(out, x, n, K, j);
  KCHECK();
}

// fam: 0 the short-row kernels, 1 the long-row ones
#define VN_LAUNCH(SHORT, WAVE, n_, ...)                                                        \
  do {                                                                                         \
    if (fam == 0) {                                                                            \
      const int g_ = vn_block_grid(n_);                                                        \
      if (K == 8) SHORT<8><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                             \
      else if (K == 4) SHORT<4><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                        \
      else SHORT<2><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                                    \
    } else {                                                                                   \
      const int g_ = vn_wave_grid(n_, K);                                                      \
      if (K == 8) WAVE<8><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                              \
      else if (K == 4) WAVE<4><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                         \
      else WAVE<2><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                                     \
    }                                                                                          \
    KCHECK();                                                                                  \
  } while (0)
static inline bool vn_k_ok(int K) { return K == 2 || K == 4 || K == 8; }
extern "C" void amgd_vcn_restrict(int fam, int K, const dcsr *Wt, const double *bF, double *bC) {
  if (!Wt->rn || !vn_k_ok(K)) return;
  VN_LAUNCH(k_vcn_restrict, k_vcn_restrict_wave, Wt->rn, Wt->ro, Wt->col, Wt->a, Wt->rn, bF, bC);
}
extern "C" void amgd_vcn_prolong(int fam, int K, const dcsr *W, const dcsr *AfP, const double *D,
                                 const double *xc, double *xf, double *bf, double *c, int add) {
  if (!W->rn || !vn_k_ok(K)) return;
  VN_LAUNCH(k_vcn_prolong, k_vcn_prolong_wave, W->rn, W->ro, W->col, W->a, AfP->ro, AfP->col, AfP->a, D, W->rn,
            xc, xf, bf, c, add);
}
extern "C" void amgd_vcn_cheb(int fam, int K, const dcsr *Af, const double *D, const double *bf, const double *c,
                              double *cn, double beta, double gamma, int has_prev, double *xf) {
  if (!Af->rn || !vn_k_ok(K)) return;
  VN_LAUNCH(k_vcn_cheb, k_vcn_cheb_wave, Af->rn, Af->ro, Af->col, Af->a, D, Af->rn, bf, c, cn, beta, gamma,
            has_prev, xf);
}
