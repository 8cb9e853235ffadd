// amgd_solve.hip -- the V-cycle's own kernels (driver: amgd_vcycle.c; contract: DESIGN.md
// "Solve").  Every product is the reference's apply_M row sum (amg_tools.c:77-99): the
// products a_ij * x_j added left to right from +0, no FMA (-ffp-contract=off), then
// alpha*y + beta*t with alpha, beta = +-1 -- so each kernel here gives the bits the composed
// path (amgd_spmv + the vector kernels) gives, which the tests hold it to.
//
// Each kernel comes as a thread-per-row form (mean row below WAVE_ROWS_MIN_MEAN) and a
// cooperative long-row form (second half of the file); the one-workgroup coarse tail runs
// the deepest levels in a single launch.  A matrix with an outlier row takes the composed
// path (amgd_vcycle.c routes and counts: vc_thr / vc_wave / vc_comp / vc_tail).
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"

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

// Short rows (mean below WAVE_ROWS_MIN_MEAN): one thread adds each row, and the loads are
// shared -- k_spmv's structure (amgd_sparse.hip).  A 256-thread block owns 256 consecutive
// rows and walks their entry range in chunks of VC_CH: all threads form the chunk's products
// with coalesced loads of (value, column) into LDS, then each thread adds the part of its
// own row inside the chunk, in order.  Chunks are visited in order, so every row sum is the
// reference's left-to-right sum from +0 whatever the row lengths.  (A plain loop of one
// thread over its row reads the matrix uncoalesced and measured slower than the composed
// path: DESIGN.md "Solve".)
#define VC_ROWS 256
#define VC_CH 4096
// the ordered sum of row i (own: i < r1) of the block's rows [r0, r1); every thread calls it
__device__ __forceinline__ double vc_block_rows(double *pv, const uint64_t *ro, const uint32_t *col,
                                                const double *a, const double *x, uint64_t r0,
                                                uint64_t r1, uint64_t i, bool own) {
  const int tid = threadIdx.x;
  const uint64_t b0 = ro[r0], b1 = ro[r1];
  const uint64_t k0 = own ? ro[i] : 0, k1 = own ? ro[i + 1] : 0;
  double t = 0.0;
  for (uint64_t c0 = b0; c0 < b1; c0 += VC_CH) {
    const uint64_t c1 = min(b1, c0 + VC_CH);
    for (uint64_t kb = c0 + tid; kb < c1; kb += 256 * 8) {
      double av[8];
      uint32_t cv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const uint64_t k = kb + 256 * u;
        av[u] = 0.0;
        cv[u] = 0;
        if (k < c1) {
          av[u] = a[k];
          cv[u] = col[k];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const uint64_t k = kb + 256 * u;
        if (k < c1) pv[k - c0] = av[u] * x[cv[u]];
      }
    }
    __syncthreads();
    const uint64_t lo = max(k0, c0), hi = min(k1, c1);
#pragma unroll 8
    for (uint64_t k = lo; k < hi; k++) t += pv[k - c0];
    __syncthreads();
  }
  return t;
}
#define VC_BLOCK_LOOP(n)                                                                       \
  for (uint64_t r0 = (uint64_t)blockIdx.x * VC_ROWS; r0 < (n); r0 += (uint64_t)gridDim.x * VC_ROWS)
static inline int vc_block_grid(uint32_t n) {
  const uint64_t g = ((uint64_t)n + VC_ROWS - 1) / VC_ROWS;
  return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

// b_{l+1} = 1*b_{l+1} + 1*(W' b_l[F]) (amg.c:125-126), in place on the tail of the flat b:
// row c of Wt reads the F slice only and writes position c of the coarse slice alone
__global__ __launch_bounds__(256) void k_vc_restrict(const uint64_t *ro, const uint32_t *col,
                                                     const double *a, uint32_t nc, const double *bF,
                                                     double *bC) {
  __shared__ double pv[VC_CH];
  VC_BLOCK_LOOP(nc) {
    const uint64_t r1 = min((uint64_t)nc, r0 + VC_ROWS), c = r0 + threadIdx.x;
    const bool own = c < r1;
    const double t = vc_block_rows(pv, ro, col, a, bF, r0, r1, c, own);
    if (own) bC[c] = bC[c] + t;
  }
}
// the same sum for a rank's own C rows (partitioned cycle): row c writes position map[c] of
// the flat b -- the own C points are not contiguous in positions
__global__ __launch_bounds__(256) void k_vc_restrict_map(const uint64_t *ro, const uint32_t *col,
                                                         const double *a, uint32_t nc, const double *bF,
                                                         double *b, const uint32_t *map) {
  __shared__ double pv[VC_CH];
  VC_BLOCK_LOOP(nc) {
    const uint64_t r1 = min((uint64_t)nc, r0 + VC_ROWS), c = r0 + threadIdx.x;
    const bool own = c < r1;
    const double t = vc_block_rows(pv, ro, col, a, bF, r0, r1, c, own);
    if (own) {
      const uint32_t q = map[c];
      b[q] = b[q] + t;
    }
  }
}
extern "C" void amgd_vc_restrict_map_thr(const dcsr *Wt, const double *bF, double *b, const uint32_t *map) {
  if (!Wt->rn) return;
  k_vc_restrict_map<<<vc_block_grid(Wt->rn), 256, 0, amgd_s()>>>(Wt->ro, Wt->col, Wt->a, Wt->rn, bF, b, map);
  KCHECK();
}
__global__ void k_vc_add_map(double *b, const uint32_t *map, const double *t, uint64_t n) {
  GRID_STRIDE(c, n) {
    const uint32_t q = map[c];
    b[q] = b[q] + t[c];
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
extern "C" void amgd_vc_restrict_thr(const dcsr *Wt, const double *bF, double *bC) {
  if (!Wt->rn) return;
  k_vc_restrict<<<vc_block_grid(Wt->rn), 256, 0, amgd_s()>>>(Wt->ro, Wt->col, Wt->a, Wt->rn, bF, bC);
  KCHECK();
}

// per F row: xf = W xc; bf = b - AfP xc; c = D.*bf; m == 1: xf += c (amg.c:142-146, :166):
// the row of W and the row of AfP against the same xc in one launch
__global__ __launch_bounds__(256) void k_vc_prolong(const uint64_t *wro, const uint32_t *wcol,
                                                    const double *wa, const uint64_t *pro,
                                                    const uint32_t *pcol, const double *pa,
                                                    const double *D, uint32_t nf, const double *xc,
                                                    double *xf, double *bf, double *c, int add) {
  __shared__ double pv[VC_CH];
  VC_BLOCK_LOOP(nf) {
    const uint64_t r1 = min((uint64_t)nf, r0 + VC_ROWS), i = r0 + threadIdx.x;
    const bool own = i < r1;
    const double xw = vc_block_rows(pv, wro, wcol, wa, xc, r0, r1, i, own);
    const double tp = vc_block_rows(pv, pro, pcol, pa, xc, r0, r1, i, own);
    if (own) {
      const double bb = bf[i] - tp;
      const double cc = D[i] * bb;
      bf[i] = bb;
      c[i] = cc;
      xf[i] = add ? xw + cc : xw;
    }
  }
}
extern "C" void amgd_vc_prolong_thr(const dcsr *W, const dcsr *AfP, const double *D, const double *xc,
                                    double *xf, double *bf, double *c, int add) {
  if (!W->rn) return;
  k_vc_prolong<<<vc_block_grid(W->rn), 256, 0, amgd_s()>>>(W->ro, W->col, W->a, AfP->ro, AfP->col, AfP->a,
                                                           D, W->rn, xc, xf, bf, c, add);
  KCHECK();
}

// one Chebyshev step in one pass over Af, no r vector: row i reads c at its columns and
// writes index i of the other buffer only (amg.c:152-155, :161-164; the last step adds
// into xf, amg.c:166)
__global__ __launch_bounds__(256) void k_vc_cheb(const uint64_t *ro, const uint32_t *col,
                                                 const double *a, const double *D, uint32_t nf,
                                                 const double *bf, const double *cg, const double *c,
                                                 double *cn, double beta, double gamma, int has_prev,
                                                 double *xf) {
  __shared__ double pv[VC_CH];
  VC_BLOCK_LOOP(nf) {
    const uint64_t r1 = min((uint64_t)nf, r0 + VC_ROWS), i = r0 + threadIdx.x;
    const bool own = i < r1;
    const double t = vc_block_rows(pv, ro, col, a, cg, r0, r1, i, own);
    if (own) {
      const double r = bf[i] - t;
      double v = beta * (c[i] + D[i] * r);
      if (has_prev) v = v - gamma * cn[i];
      cn[i] = v;
      if (xf) xf[i] = xf[i] + v;
    }
  }
}
// cg: the vector the row sums gather from (Af's columns index it); c, cn, bf, D, xf: the rows'
// own entries.  One GPU: cg == c.  A rank's row block: cg the whole c, the rest offset to its rows
extern "C" void amgd_vc_cheb_thr_g(const dcsr *Af, const double *D, const double *bf, const double *cg,
                                   const double *c, double *cn, double beta, double gamma, int has_prev,
                                   double *xf) {
  if (!Af->rn) return;
  k_vc_cheb<<<vc_block_grid(Af->rn), 256, 0, amgd_s()>>>(Af->ro, Af->col, Af->a, D, Af->rn, bf, cg, c, cn, beta,
                                                         gamma, has_prev, xf);
  KCHECK();
}
extern "C" void amgd_vc_cheb_thr(const dcsr *Af, const double *D, const double *bf, const double *c,
                                 double *cn, double beta, double gamma, int has_prev, double *xf) {
  amgd_vc_cheb_thr_g(Af, D, bf, c, c, cn, beta, gamma, has_prev, xf);
}

// The coarse tail: the deepest levels, whose flat slices together hold at most 1024
// positions, in ONE workgroup -- restriction down through them, the bottom solve, the
// up-sweep -- one thread per row and a block barrier between phases, instead of four to
// seven launches per level.  Level l's slices: F at [off, off + nf), coarse at
// [off + nf, N).  Same row sums and the same scalar sequence (beta / gamma from the host)
// as the per-level kernels.
__global__ __launch_bounds__(1024) void k_vc_tail(const amgd_vc_tlev *lv, int nl, double *b, double *x,
                                                  double *c0, double *c1, uint32_t N, double dbot,
                                                  int up_only) {
  const uint32_t t = threadIdx.x;
  if (!up_only) {
    for (int l = 0; l < nl; l++) {
      const amgd_vc_tlev *L = &lv[l];
      if (t < L->nc) {
        double *bC = b + L->off + L->nf;
        bC[t] = bC[t] + vc_row(L->wt_ro, L->wt_col, L->wt_a, b + L->off, t);
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
      const double bb = bf[t] - vc_row(L->p_ro, L->p_col, L->p_a, xc, t);
      const double cc = L->D[t] * bb;
      bf[t] = bb;
      c[t] = cc;
      xf[t] = L->steps == 0 ? xw + cc : xw;
    }
    __syncthreads();
    for (uint32_t k = 0; k < L->steps; k++) {
      if (t < L->nf) {
        const double r = bf[t] - vc_row(L->af_ro, L->af_col, L->af_a, c, t);
        double v = L->beta[k] * (c[t] + L->D[t] * r);
        if (k > 0) v = v - L->gamma[k] * cn[t];
        cn[t] = v;
        if (k + 1 == L->steps) xf[t] = xf[t] + v;
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
// Cooperative long-row form (mean row >= WAVE_ROWS_MIN_MEAN), after k_spmv_pipe's structure
// (amgd_sparse.hip): a wavefront owns RW rows and walks them in rounds of SEG = 64 PER / RW
// entries per row.  A round's (value, column) pairs are loaded coalesced -- each load
// instruction covers whole row segments -- multiplied with the gathered x and staged in an
// LDS tile; lane r of the first RW then adds row r's segment left to right, so every row
// sum is the reference's ordered sum from +0.  The wavefront-scope fences and barriers
// around the tile are required exactly as there: the tile is written by all 64 lanes and
// read by other lanes of the same wavefront.  Unlike k_spmv_pipe the next round's loads are
// not issued ahead of the adds; a lane past its row's end loads nothing.
// RW by row count like the setup's lane kernel: 4 below 2^16 rows, 16 below 2^22, else 64.
// ---------------------------------------------------------------------------
template <int RW, int PER> struct VcTile {
  static constexpr int SEG = 64 * PER / RW;
  double buf[4][RW][SEG + 1];
  uint64_t rk0[4][RW];
  uint32_t rlen[4][RW];
};
__device__ __forceinline__ void vc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ordered sums of rows rb .. rb + RW - 1 (those < n) against x; lane r < RW returns row
// rb + r's sum.  Every lane of the wavefront calls it.
template <int RW, int PER>
__device__ __forceinline__ double vc_coop_rows(VcTile<RW, PER> &T, const uint64_t *ro, const uint32_t *col,
                                               const double *a, const double *x, uint64_t rb, uint32_t n) {
  constexpr int SEG = VcTile<RW, PER>::SEG;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t r = rb + lane;
  const bool own = lane < RW && r < n;
  const uint64_t k0 = own ? ro[r] : 0, k1 = own ? ro[r + 1] : 0;
  const uint32_t len = (uint32_t)(k1 - k0);
  vc_wave_sync();                          // the previous call's tile reads are done
  if (lane < RW) {
    T.rk0[w][lane] = k0;
    T.rlen[w][lane] = len;
  }
  uint32_t mx = len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(mx, o, 64); mx = u > mx ? u : mx; }
  vc_wave_sync();
  double t = 0.0;
  for (uint32_t off = 0; off < mx; off += SEG) {
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int fl = q * 64 + lane, rr = fl / SEG, sub = fl % SEG;
      const uint32_t en = off + sub;
      double pr = 0.0;
      if (en < T.rlen[w][rr]) {
        const uint64_t k = T.rk0[w][rr] + en;
        pr = a[k] * x[col[k]];
      }
      T.buf[w][rr][sub] = pr;
    }
    vc_wave_sync();
    if (lane < RW && off < len) {
      const uint32_t m = min((uint32_t)SEG, len - off);
      for (uint32_t e = 0; e < m; e++) t += T.buf[w][lane][e];
    }
    vc_wave_sync();
  }
  return t;
}

template <int RW, int PER>
__global__ __launch_bounds__(256) void k_vc_restrict_coop(const uint64_t *ro, const uint32_t *col,
                                                          const double *a, uint32_t nc, const double *bF,
                                                          double *bC) {
  __shared__ VcTile<RW, PER> T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t rb = ((uint64_t)blockIdx.x * 4 + w) * RW; rb < nc; rb += (uint64_t)gridDim.x * 4 * RW) {
    const double t = vc_coop_rows<RW, PER>(T, ro, col, a, bF, rb, nc);
    const uint64_t c = rb + lane;
    if (lane < RW && c < nc) bC[c] = bC[c] + t;
  }
}
template <int RW, int PER>
__global__ __launch_bounds__(256) void k_vc_restrict_map_coop(const uint64_t *ro, const uint32_t *col,
                                                              const double *a, uint32_t nc, const double *bF,
                                                              double *b, const uint32_t *map) {
  __shared__ VcTile<RW, PER> T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t rb = ((uint64_t)blockIdx.x * 4 + w) * RW; rb < nc; rb += (uint64_t)gridDim.x * 4 * RW) {
    const double t = vc_coop_rows<RW, PER>(T, ro, col, a, bF, rb, nc);
    const uint64_t c = rb + lane;
    if (lane < RW && c < nc) {
      const uint32_t q = map[c];
      b[q] = b[q] + t;
    }
  }
}
template <int RW, int PER>
__global__ __launch_bounds__(256) void k_vc_prolong_coop(const uint64_t *wro, const uint32_t *wcol,
                                                         const double *wa, const uint64_t *pro,
                                                         const uint32_t *pcol, const double *pa,
                                                         const double *D, uint32_t nf, const double *xc,
                                                         double *xf, double *bf, double *c, int add) {
  __shared__ VcTile<RW, PER> T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t rb = ((uint64_t)blockIdx.x * 4 + w) * RW; rb < nf; rb += (uint64_t)gridDim.x * 4 * RW) {
    const double xw = vc_coop_rows<RW, PER>(T, wro, wcol, wa, xc, rb, nf);
    const double tp = vc_coop_rows<RW, PER>(T, pro, pcol, pa, xc, rb, nf);
    const uint64_t i = rb + lane;
    if (lane < RW && i < nf) {
      const double bb = bf[i] - tp;
      const double cc = D[i] * bb;
      bf[i] = bb;
      c[i] = cc;
      xf[i] = add ? xw + cc : xw;
    }
  }
}
template <int RW, int PER>
__global__ __launch_bounds__(256) void k_vc_cheb_coop(const uint64_t *ro, const uint32_t *col,
                                                      const double *a, const double *D, uint32_t nf,
                                                      const double *bf, const double *cg, const double *c,
                                                      double *cn, double beta, double gamma, int has_prev,
                                                      double *xf) {
  __shared__ VcTile<RW, PER> T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t rb = ((uint64_t)blockIdx.x * 4 + w) * RW; rb < nf; rb += (uint64_t)gridDim.x * 4 * RW) {
    const double t = vc_coop_rows<RW, PER>(T, ro, col, a, cg, rb, nf);
    const uint64_t i = rb + lane;
    if (lane < RW && i < nf) {
      const double r = bf[i] - t;
      double v = beta * (c[i] + D[i] * r);
      if (has_prev) v = v - gamma * cn[i];
      cn[i] = v;
      if (xf) xf[i] = xf[i] + v;
    }
  }
}
static inline int vc_rw(uint64_t n) {
  const int64_t rw = amgd_knob(AMGD_K_VC_RW);   // tests: 4 / 16 / 64 forces the shape, else by row count
  if (rw == 4 || rw == 16 || rw == 64) return (int)rw;
  return n >= (1ull << 22) ? 64 : n >= (1ull << 16) ? 16 : 4;
}
static inline int vc_grid(uint64_t n, int rw) {
  const uint64_t g = (n + 4ull * rw - 1) / (4ull * rw);
  return (int)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}
#define VC_COOP_LAUNCH(KERNEL, n_, ...)                                                        \
  do {                                                                                         \
    const int rw_ = vc_rw(n_);                                                                 \
    const int g_ = vc_grid(n_, rw_);                                                           \
    if (rw_ == 64) KERNEL<64, 16><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                      \
    else if (rw_ == 16) KERNEL<16, 16><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                 \
    else KERNEL<4, 8><<<g_, 256, 0, amgd_s()>>>(__VA_ARGS__);                                  \
    KCHECK();                                                                                  \
  } while (0)
extern "C" void amgd_vc_restrict_coop(const dcsr *Wt, const double *bF, double *bC) {
  if (!Wt->rn) return;
  VC_COOP_LAUNCH(k_vc_restrict_coop, Wt->rn, Wt->ro, Wt->col, Wt->a, Wt->rn, bF, bC);
}
extern "C" void amgd_vc_prolong_coop(const dcsr *W, const dcsr *AfP, const double *D, const double *xc,
                                     double *xf, double *bf, double *c, int add) {
  if (!W->rn) return;
  VC_COOP_LAUNCH(k_vc_prolong_coop, W->rn, W->ro, W->col, W->a, AfP->ro, AfP->col, AfP->a, D, W->rn, xc,
                 xf, bf, c, add);
}
extern "C" void amgd_vc_restrict_map_coop(const dcsr *Wt, const double *bF, double *b, const uint32_t *map) {
  if (!Wt->rn) return;
  VC_COOP_LAUNCH(k_vc_restrict_map_coop, Wt->rn, Wt->ro, Wt->col, Wt->a, Wt->rn, bF, b, map);
}
extern "C" void amgd_vc_cheb_coop_g(const dcsr *Af, const double *D, const double *bf, const double *cg,
                                    const double *c, double *cn, double beta, double gamma, int has_prev,
                                    double *xf) {
  if (!Af->rn) return;
  VC_COOP_LAUNCH(k_vc_cheb_coop, Af->rn, Af->ro, Af->col, Af->a, D, Af->rn, bf, cg, c, cn, beta, gamma,
                 has_prev, xf);
}
extern "C" void amgd_vc_cheb_coop(const dcsr *Af, const double *D, const double *bf, const double *c,
                                  double *cn, double beta, double gamma, int has_prev, double *xf) {
  amgd_vc_cheb_coop_g(Af, D, bf, c, c, cn, beta, gamma, has_prev, xf);
}
