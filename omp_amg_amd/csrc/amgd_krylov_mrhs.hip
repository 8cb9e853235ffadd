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
// Two row shapes, the row-sum device functions of the K-column V-cycle (amgd_mrhs_dev.h):
//   k_kry_spmv_n       short rows: a block owns 256 consecutive rows and stages their (value,
//                      column) pairs in LDS chunk by chunk; the row's thread adds its K sums
//   k_kry_spmv_n_wave  long rows: a wavefront owns 64 / K rows, rounds of 16 entries per row,
//                      the K products of an entry staged in an LDS tile, lane r*K + j adds
//                      column j of row r
#include <hip/hip_runtime.h>

#include "amgd.h"
#include "amgd_dev.h"
#include "amgd_mrhs_dev.h"

// column j's pointer out of a by-value table, j not uniform over the wavefront: a chain of
// selects, never an indexed read of private memory
template <int K, typename P, typename T> __device__ __forceinline__ P kry_pick(const T &tab, int j) {
  P p = tab.p[0];
#pragma unroll
  for (int q = 1; q < K; q++) p = j == q ? tab.p[q] : p;
  return p;
}

template <int K>
__global__ __launch_bounds__(256) void k_kry_spmv_n(const uint64_t *__restrict__ ro, const uint32_t *__restrict__ col,
                                                    const double *__restrict__ a, uint32_t n,
                                                    const double *__restrict__ xi, amgd_ptr8 z, double alpha,
                                                    amgd_cptr8 y, int has_y, double beta) {
  __shared__ double sa[VN_CH];
  __shared__ uint32_t sc[VN_CH];
  VN_BLOCK_LOOP(n) {
    const uint64_t r1 = min((uint64_t)n, r0 + VN_ROWS), i = r0 + threadIdx.x;
    const bool own = i < r1;
    const VecK<K> t = vn_block_rows<K>(sa, sc, ro, col, a, xi, r0, r1, i, own);
    if (own) {
#pragma unroll
      for (int j = 0; j < K; j++) z.p[j][i] = has_y ? alpha * y.p[j][i] + beta * t.v[j] : beta * t.v[j];
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void k_kry_spmv_n_wave(const uint64_t *__restrict__ ro,
                                                         const uint32_t *__restrict__ col,
                                                         const double *__restrict__ a, uint32_t n,
                                                         const double *__restrict__ xi, amgd_ptr8 z, double alpha,
                                                         amgd_cptr8 y, int has_y, double beta) {
  __shared__ VnTile<K> T;
  const int lane = threadIdx.x & 63, lj = lane % K;
  double *zp = kry_pick<K, double *>(z, lj);
  const double *yp = kry_pick<K, const double *>(y, lj);
  VN_WAVE_LOOP(n) {
    const double t = vn_coop_rows<K>(T, ro, col, a, xi, rb, n);
    const uint64_t i = rb + lane / K;
    if (i < n) zp[i] = has_y ? alpha * yp[i] + beta * t : beta * t;
  }
}

extern "C" void amgd_kry_spmv_n(const dcsr *A, int K, int fam, const amgd_cptr8 *x, const amgd_ptr8 *z,
                                double alpha, const amgd_cptr8 *y, double beta, double *xi) {
  if (!A->rn || (K != 2 && K != 4 && K != 8)) return;
  amgd_vcn_scatter(xi, x, nullptr, A->cn, K);
  const int has_y = !(alpha == 0.0 || y == nullptr);
  const amgd_cptr8 Y = amgd_cptr8_of(has_y ? y->p : nullptr, has_y ? K : 0);
  hipStream_t st = amgd_s();
#define KRY_SPMV_ARGS A->ro, A->col, A->a, A->rn, xi, *z, alpha, Y, has_y, beta
  if (fam == 0) {
    const int g = vn_block_grid(A->rn);
    if (K == 8) k_kry_spmv_n<8><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
    else if (K == 4) k_kry_spmv_n<4><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
    else k_kry_spmv_n<2><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
  } else {
    const int g = vn_wave_grid(A->rn, K);
    if (K == 8) k_kry_spmv_n_wave<8><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
    else if (K == 4) k_kry_spmv_n_wave<4><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
    else k_kry_spmv_n_wave<2><<<g, 256, 0, st>>>(KRY_SPMV_ARGS);
  }
#undef KRY_SPMV_ARGS
  KCHECK();
}
