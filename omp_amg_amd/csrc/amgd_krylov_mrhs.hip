// amgd_krylov_mrhs.hip -- the level-0 product of the multi-RHS Krylov solver for a group of
// K = 2, 4 or 8 columns given by pointer (driver amgd_krylov.c, amgd_krylov_device_n; DESIGN.md
// "Krylov on several right-hand sides").
//
//   z_j = alpha*y_j + beta*(A x_j), j < K        (alpha == 0 or no y: z_j = beta*(A x_j))
//
// A's (value, column) stream is read ONCE for the K columns.  The operands are interleaved
// first, element (row q, column j) at xi[q*K + j] (one copy of 16 K n bytes, counted in the
// driver's byte figure), so an entry's K operands are one contiguous 8K-byte read; the results
// go straight to the columns' own vectors.  Every (row, column) sum is amgd_spmv's: the row's
// products a_ik * x_kj added left to right from +0.0, each rounded before it is added (no FMA:
// -ffp-contract=off), and the last expression is amgd_spmv's as written there -- column j comes
// out bit for bit as amgd_spmv gives it, whatever K and whichever row shape.
//
// Two row shapes, the K-column row-sum policies of the V-cycle (amgd_vc_dev.h):
//   k_kry_spmv_n<VnBlock<K>>  short rows: a block owns 256 consecutive rows and stages their
//                      (value, column) pairs in LDS chunk by chunk; the row's thread adds its K sums
//   k_kry_spmv_n<VnCoop<K>>   long rows: a wavefront owns 64 / K rows, rounds of 16 entries per
//                      row, the K products of an entry staged in an LDS tile, lane r*K + j adds
//                      column j of row r
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"
#include "amgd_vc_dev.h"

// column j's pointer out of a by-value table, j not uniform over the wavefront: a chain of
// selects, never an indexed read of private memory
template <int K, typename P, typename T> __device__ __forceinline__ P kry_pick(const T &tab, int j) {
  P p = tab.p[0];
#pragma unroll
  for (int q = 1; q < K; q++) p = j == q ? tab.p[q] : p;
  return p;
}

// one kernel over the two K-column policies; a VnBlock thread writes its row of all K columns,
// a VnCoop lane its row of column lane % K
template <class P>
__global__ __launch_bounds__(256) void k_kry_spmv_n(const uint64_t *__restrict__ ro, const uint32_t *__restrict__ col,
                                                    const double *__restrict__ a, uint32_t n,
                                                    const double *__restrict__ xi, amgd_ptr8 z, double alpha,
                                                    amgd_cptr8 y, int has_y, double beta) {
  constexpr int K = P::Cols;
  __shared__ typename P::Shared S;
  const int lj = (threadIdx.x & 63) % K;
  double *zp = P::OWN == 1 ? kry_pick<K, double *>(z, lj) : nullptr;
  const double *yp = P::OWN == 1 ? kry_pick<K, const double *>(y, lj) : nullptr;
  for (uint64_t g = P::first(); g < n; g += P::stride()) {
    const VecK<P::OWN> t = P::rows(S, ro, col, a, xi, g, n);
    if (P::owns(g, n)) {
      const uint64_t i = P::row(g);
      if constexpr (P::OWN == 1) {
        zp[i] = has_y ? alpha * yp[i] + beta * t.v[0] : beta * t.v[0];
      } else {
#pragma unroll
        for (int j = 0; j < P::OWN; j++) z.p[j][i] = has_y ? alpha * y.p[j][i] + beta * t.v[j] : beta * t.v[j];
      }
    }
  }
}

extern "C" void amgd_kry_spmv_n(const dcsr *A, int K, int fam, const amgd_cptr8 *x, const amgd_ptr8 *z,
                                double alpha, const amgd_cptr8 *y, double beta, double *xi) {
  if (!A->rn || (K != 2 && K != 4 && K != 8)) return;
  amgd_vcn_scatter(xi, x, nullptr, A->cn, K);
  const int has_y = !(alpha == 0.0 || y == nullptr);
  const amgd_cptr8 Y = amgd_cptr8_of(has_y ? y->p : nullptr, has_y ? K : 0);
#define KRY_GO(P) k_kry_spmv_n<P><<<P::grid(A->rn), 256, 0, amgd_s()>>>(A->ro, A->col, A->a, A->rn, xi, *z, alpha, Y, has_y, beta)
  if (fam == 0) {
    if (K == 8) KRY_GO(VnBlock<8>);
    else if (K == 4) KRY_GO(VnBlock<4>);
    else KRY_GO(VnBlock<2>);
  } else {
    if (K == 8) KRY_GO(VnCoop<8>);
    else if (K == 4) KRY_GO(VnCoop<4>);
    else KRY_GO(VnCoop<2>);
  }
#undef KRY_GO
  KCHECK();
}
