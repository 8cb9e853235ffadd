// amgd_solve_mrhs.hip -- the layout kernels of the V-cycle for a group of K = 2, 4 or 8
// right-hand sides (driver: amgd_vcycle.c, "several right-hand sides"; contract: DESIGN.md
// "Solve").
//
// Layout: the K vectors of a group are interleaved, element (position q, column j) at q*K + j,
// so a row's thread loads each (value, column) pair ONCE for K products and gathers the K
// operands of an entry with one contiguous 8K-byte read.  The level operations themselves are
// the kernel templates of amgd_solve.hip over the K-column row-sum policies (amgd_vc_dev.h);
// here are the copies into and out of the layout, the bottom solve and one column in or out
// (a level whose matrix has an outlier row runs column by column through the single-vector code).
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"
#include "amgd_vc_dev.h"

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
